"""Hyperelastic tangent and forces on the GPU (fedd_assemble_hyperelastic) against the numpy restatement of
tests/hyperelastic_ref.py, the properties of the forms, and Newton's method run at the ABI level: assembly, Dirichlet rows,
Schwarz and GMRES on the device, the loop itself on the host."""
import os

import numpy as np
import pytest

import hyperelastic_ref as hr
from test_gpu_parity import csr_global

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
RTOL = 1e-10        # the project's parity bar

# the reference's parametersProblem.xml: E = 1, nu = 0.4, Mu = 0.3571, C = 1
PARAMS = {hr.NEOHOOKE: (1.0, 0.4), hr.MOONEY_RIVLIN: (1.0, 0.4, 1.0), hr.STVK: hr.stvk_params(0.3571, 0.4)}
PARAMS_B = {hr.NEOHOOKE: (3.0e6, 0.3), hr.MOONEY_RIVLIN: (2.5, 0.3, 0.35), hr.STVK: (1.5, 0.8)}


def model_id(lib, model):
    return {hr.NEOHOOKE: lib.HYPER_NEOHOOKE, hr.MOONEY_RIVLIN: lib.HYPER_MOONEY_RIVLIN, hr.STVK: lib.HYPER_STVK}[model]


MESHES = ["p1_cube3", "p1_cube5", "p2_cube2", "p2_cube3", "p2_tet", "p1_square4", "p2_square4"]
_mesh_cache = {}


def mesh(lib, which):
    """p1_cube3: corner, edge, face and interior nodes; p1_cube5: 750 elements, several workgroups and a partial last one;
    p2_cube3: 162 elements, not a multiple of a workgroup's four; p2_tet: the single tetrahedron of tests/golden"""
    if which not in _mesh_cache:
        if which == "p2_tet":
            m = lib.p2_of_p1(lib.read_mesh(os.path.join(GOLD, "tetrahedron.mesh"), 3), volume_id=0)
        else:
            fe, shape = which.split("_")
            dim = 3 if shape.startswith("cube") else 2
            m = lib.structured_mesh(dim, 1, int(shape[-1]))
            if fe == "p2":      # the mid nodes of the boundary take their flags from the surface elements
                m["surf"], m["surf_flag"] = lib.structured_surfaces(dim, 1, int(shape[-1]))
                m = lib.p2_of_p1(m, volume_id=0)
        _mesh_cache[which] = m
    return _mesh_cache[which]


def models_of(m):
    return hr.MODELS if m["dim"] == 3 else (hr.STVK,)


def mesh_size(m):
    X = m["xyz"][m["conn"][:, :m["dim"] + 1]]
    return np.linalg.norm(X[:, 1:] - X[:, :1], axis=2).min()


def smooth_displacement(m, seed=7, scale=0.08):
    """smooth, not a polynomial, plus a seeded perturbation of amplitude 0.05 h; [n_global, dim]"""
    n, dim = int(m["n_global"]), m["dim"]
    x = np.zeros((n, dim))
    x[m["gid_rep"]] = m["xyz"]
    s = x.sum(axis=1)
    cols = [np.sin(1.3 * x[:, 0] + 0.4 * s), np.cos(0.9 * x[:, 1] - 0.7 * s) * np.exp(0.3 * x[:, 0]) - 1.0]
    if dim == 3:
        cols.append(np.sin(1.1 * x[:, 2]) * np.cos(0.8 * s))
    u = scale * np.stack(cols, axis=1)
    return u + 0.05 * mesh_size(m) * np.random.default_rng(seed).uniform(-1.0, 1.0, u.shape)


@pytest.fixture()
def ctx(fedd_lib):
    c = fedd_lib.Context(device=0)
    yield c
    c.close()


def own_dofs(m):
    return (m["dim"] * np.asarray(m["gid_uni"], dtype=np.int64)[:, None] + np.arange(m["dim"])[None, :]).ravel()


def setup(lib, ctx, m):
    ctx.mesh_set_dict(m)
    ctx.pattern_build(m["dim"], lib.BLOCK_FULL)


def gpu_assemble(lib, ctx, m, u_glob, model, params, what=3):
    """(K in global ids | None, f in global ids | None) of one device call"""
    dim = m["dim"]
    ctx.velocity_set(np.asarray(u_glob).reshape(-1, dim)[m["gid_rep"]])
    ctx.assemble_hyperelastic(model_id(lib, model), params, what)
    K = f = None
    if what & lib.HYPER_TANGENT:
        K = csr_global(ctx, dim * int(m["n_global"]))[0]
    if what & lib.HYPER_FORCE:
        f = np.zeros(dim * int(m["n_global"]))
        f[own_dofs(m)] = ctx.hyperelastic_force_get()
    return K, f


def assert_tangent_close(A, B):
    A = A.tocsr(); B = B.tocsr()
    A.sort_indices(); B.sort_indices()
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices)      # the pattern, structural zeros included
    scale = np.abs(B).max(axis=1).toarray().ravel()
    assert scale.min() > 0.0
    err = np.abs(A.data - B.data) / np.repeat(scale, np.diff(B.indptr))
    assert err.max() <= RTOL, err.max()
    return err.max()


@pytest.fixture(scope="module")
def reference():
    """restatement results, computed once per (mesh, model, parameter set) and shared"""
    cache = {}

    def get(lib, which, model, params, u):
        key = (which, model, tuple(params))
        if key not in cache:
            m = mesh(lib, which)
            cache[key] = hr.assemble(m, u.reshape(-1, m["dim"])[m["gid_rep"]], model, params)
        return cache[key]
    return get


@pytest.mark.parametrize("which", MESHES)
def test_tangent_and_force_match_the_restatement(fedd_lib, ctx, reference, which):
    m = mesh(fedd_lib, which)
    u = smooth_displacement(m)
    setup(fedd_lib, ctx, m)
    for model in models_of(m):
        for params in (PARAMS[model], PARAMS_B[model]):
            K0, f0, minJ = reference(fedd_lib, which, model, params, u)
            assert minJ > 0.5, minJ             # a condition on the inputs: far from the ln J singularity
            K, f = gpu_assemble(fedd_lib, ctx, m, u, model, params)
            ek = assert_tangent_close(K, K0)
            ef = np.abs(f - f0).max() / np.abs(f0).max()
            print("%s %s: min J %.3f, tangent %.2e of the row maximum, force %.2e of its maximum" % (which, model, minJ, ek, ef))
            assert ef <= RTOL


@pytest.mark.parametrize("which", ["p1_cube3", "p2_cube2", "p2_tet", "p1_square4", "p2_square4"])
def test_zero_displacement_gives_no_force_and_the_linear_elastic_matrix(fedd_lib, ctx, which):
    m = mesh(fedd_lib, which)
    setup(fedd_lib, ctx, m)
    u = np.zeros((int(m["n_global"]), m["dim"]))
    for model in models_of(m):
        K, f = gpu_assemble(fedd_lib, ctx, m, u, model, PARAMS[model])
        assert np.all(f == 0.0), model                                  # exactly
        if model == hr.MOONEY_RIVLIN:
            continue
        lam, mu = PARAMS[model] if model == hr.STVK else hr.lame(*PARAMS[model])[::-1]
        ctx.assemble(fedd_lib.FORM_LINELAS, [lam, mu])
        L = csr_global(ctx, K.shape[0])[0]
        assert_tangent_close(K, L)


@pytest.mark.parametrize("which", ["p1_cube3", "p2_cube2", "p1_square4", "p2_square4"])
def test_rigid_rotation_gives_no_force(fedd_lib, ctx, which):
    """u = (R - I) x is in the P1 and P2 spaces: F = R at every point, P(R) = 0"""
    m = mesh(fedd_lib, which)
    dim = m["dim"]
    setup(fedd_lib, ctx, m)
    R = np.eye(dim)
    R[:2, :2] = [[np.cos(0.9), -np.sin(0.9)], [np.sin(0.9), np.cos(0.9)]]
    if dim == 3:
        R2 = np.eye(3)
        R2[1:, 1:] = [[np.cos(0.4), -np.sin(0.4)], [np.sin(0.4), np.cos(0.4)]]
        R = R2 @ R
    x = np.zeros((int(m["n_global"]), dim))
    x[m["gid_rep"]] = m["xyz"]
    u = x @ (R - np.eye(dim)).T
    for model in models_of(m):
        K, f = gpu_assemble(fedd_lib, ctx, m, u, model, PARAMS[model])
        knorm = np.abs(K).sum(axis=1).max()
        print("%s %s: |f| %.2e, |K| %.2e, |u| %.2e" % (which, model, np.abs(f).max(), knorm, np.abs(u).max()))
        assert np.abs(f).max() <= RTOL * knorm * np.abs(u).max()


@pytest.mark.parametrize("which", ["p1_cube3", "p2_cube2", "p2_square4"])
def test_tangent_is_the_derivative_of_the_force(fedd_lib, ctx, which):
    """(f(u + eps v) - f(u - eps v)) / (2 eps) against K(u) v through fedd_spmv, eps = 1e-6: truncation O(eps^2), rounding
    eps_machine / eps = 1e-10"""
    m = mesh(fedd_lib, which)
    dim = m["dim"]
    setup(fedd_lib, ctx, m)
    u = smooth_displacement(m)
    v = np.random.default_rng(11).uniform(-1.0, 1.0, u.shape)
    own = own_dofs(m)
    eps = 1e-6
    for model in models_of(m):
        p = PARAMS[model]
        _, fp = gpu_assemble(fedd_lib, ctx, m, u + eps * v, model, p, fedd_lib.HYPER_FORCE)
        _, fm = gpu_assemble(fedd_lib, ctx, m, u - eps * v, model, p, fedd_lib.HYPER_FORCE)
        gpu_assemble(fedd_lib, ctx, m, u, model, p, fedd_lib.HYPER_TANGENT)
        Kv = ctx.spmv(v.ravel()[own])
        fd = ((fp - fm) / (2 * eps))[own]
        err = np.abs(fd - Kv).max() / np.abs(Kv).max()
        print("%s %s: %.2e" % (which, model, err))
        assert err <= 1e-6


@pytest.mark.parametrize("which", ["p1_cube5", "p2_cube3", "p2_square4"])
def test_two_calls_give_the_same_bits_and_the_parts_those_of_the_whole(fedd_lib, ctx, which):
    m = mesh(fedd_lib, which)
    setup(fedd_lib, ctx, m)
    u = smooth_displacement(m)
    for model in models_of(m):
        p = PARAMS[model]
        K, f = gpu_assemble(fedd_lib, ctx, m, u, model, p)
        K2, f2 = gpu_assemble(fedd_lib, ctx, m, u, model, p)
        assert np.array_equal(K.data, K2.data) and np.array_equal(f, f2)
        gpu_assemble(fedd_lib, ctx, m, 0.5 * u, model, p)                       # other values in between
        Kt, _ = gpu_assemble(fedd_lib, ctx, m, u, model, p, fedd_lib.HYPER_TANGENT)
        gpu_assemble(fedd_lib, ctx, m, 0.5 * u, model, p)
        _, ff = gpu_assemble(fedd_lib, ctx, m, u, model, p, fedd_lib.HYPER_FORCE)
        assert np.array_equal(K.data, Kt.data) and np.array_equal(f, ff)


@pytest.mark.parametrize("which", ["p1_cube3", "p2_cube2"])
def test_inverted_element_is_an_error_that_leaves_the_previous_result(fedd_lib, ctx, which):
    m = mesh(fedd_lib, which)
    setup(fedd_lib, ctx, m)
    x = np.zeros((int(m["n_global"]), 3))
    x[m["gid_rep"]] = m["xyz"]
    u = smooth_displacement(m)
    for model in (hr.NEOHOOKE, hr.MOONEY_RIVLIN):
        K, f = gpu_assemble(fedd_lib, ctx, m, u, model, PARAMS[model])
        with pytest.raises(fedd_lib.FeddError, match=r"element 0 is inverted"):     # u = -2 x: F = -I everywhere, the first element is 0
            gpu_assemble(fedd_lib, ctx, m, -2.0 * x, model, PARAMS[model])
        K2 = csr_global(ctx, K.shape[0])[0]
        assert np.array_equal(K.data, K2.data)                                      # not half-overwritten: not written at all
        assert np.array_equal(f[own_dofs(m)], ctx.hyperelastic_force_get())
    # one inverted element in the middle of the mesh: named by its index
    e = m["conn"].shape[0] // 2
    ub = np.zeros_like(x)
    nodes = m["gid_rep"][m["conn"][e]]
    ub[nodes] = -2.0 * (x[nodes] - x[nodes[0]])
    with pytest.raises(fedd_lib.FeddError, match=r"element \d+ is inverted"):
        gpu_assemble(fedd_lib, ctx, m, ub, hr.NEOHOOKE, PARAMS[hr.NEOHOOKE])
    # Saint Venant-Kirchhoff is a polynomial in F: evaluated as in the reference
    # (u = -2.5 x, F = -1.5 I: at F = -I the strain and with it the force would vanish)
    K, f = gpu_assemble(fedd_lib, ctx, m, -2.5 * x, hr.STVK, PARAMS[hr.STVK])
    K0, f0, minJ = hr.assemble(m, (-2.5 * x)[m["gid_rep"]], hr.STVK, PARAMS[hr.STVK])
    assert minJ < 0.0
    assert_tangent_close(K, K0)
    assert np.abs(f - f0).max() <= RTOL * np.abs(f0).max()


def test_errors_in_the_style_of_the_neighbouring_entries(fedd_lib, ctx):
    m2, m3 = mesh(fedd_lib, "p1_square4"), mesh(fedd_lib, "p1_cube3")
    nh = (fedd_lib.HYPER_NEOHOOKE, [1.0, 0.4])
    with pytest.raises(fedd_lib.FeddError, match="fedd_mesh_set"):
        ctx.assemble_hyperelastic(*nh)
    ctx.mesh_set_dict(m3)
    with pytest.raises(fedd_lib.FeddError, match="FULL pattern"):
        ctx.assemble_hyperelastic(*nh)
    ctx.pattern_build(3, fedd_lib.BLOCK_DIAG)
    with pytest.raises(fedd_lib.FeddError, match="FULL pattern"):
        ctx.assemble_hyperelastic(*nh)
    ctx.pattern_build(3, fedd_lib.BLOCK_FULL)
    with pytest.raises(fedd_lib.FeddError, match="fedd_velocity_set"):
        ctx.assemble_hyperelastic(*nh)
    ctx.velocity_set(np.zeros((m3["xyz"].shape[0], 3)))
    with pytest.raises(fedd_lib.FeddError, match="unknown material model 7"):
        ctx.assemble_hyperelastic(7, [1.0, 0.4])
    with pytest.raises(fedd_lib.FeddError, match="takes 3 parameters"):
        ctx.assemble_hyperelastic(fedd_lib.HYPER_MOONEY_RIVLIN, [1.0, 0.4])
    with pytest.raises(fedd_lib.FeddError, match="neither tangent nor force"):
        ctx.assemble_hyperelastic(fedd_lib.HYPER_NEOHOOKE, [1.0, 0.4], 0)
    with pytest.raises(fedd_lib.FeddError, match="no fedd_assemble_hyperelastic call"):
        ctx.hyperelastic_force_get()
    ctx.assemble_hyperelastic(*nh)
    setup(fedd_lib, ctx, m2)
    ctx.velocity_set(np.zeros((m2["xyz"].shape[0], 2)))
    with pytest.raises(fedd_lib.FeddError, match="only Saint Venant-Kirchhoff in 2D"):
        ctx.assemble_hyperelastic(*nh)


def volume_rhs(lib, ctx, m, force):
    """the load vector of the reference driver's rhs2D / rhsX (main.cpp:28-50) in global ids; leaves the pattern zeroed"""
    dim = m["dim"]
    f = [0.0, force] if dim == 2 else [force, 0.0, 0.0]
    ctx.pattern_build(dim, lib.BLOCK_FULL)
    ctx.assemble_rhs(f)
    rhs = np.zeros(dim * int(m["n_global"]))
    rhs[own_dofs(m)] = ctx.rhs_get()
    return rhs


def gpu_newton(lib, ctx, m, model, params, rhs, bc_flags=(2,), tol=1e-12, max_it=25, rtol=1e-13, gmres_its=600, restart=200,
               combine=None, strict=False):
    """hyperelastic_ref.newton with every step but the loop on the device (strict: stop at ratio < tol, as NonLinearSolver does)"""
    combine = lib.COMBINE_RESTRICTED if combine is None else combine
    dim = m["dim"]
    own = own_dofs(m)
    is_dir = hr.dirichlet_mask(m, bc_flags)[own]
    u = np.zeros(rhs.shape[0])
    ratios, r0 = [], None
    for it in range(max_it + 1):
        ctx.velocity_set(u.reshape(-1, dim)[m["gid_rep"]])
        ctx.assemble_hyperelastic(model_id(lib, model), params)
        r = ctx.hyperelastic_force_get() - rhs[own]
        r[is_dir] = 0.0
        nr = np.linalg.norm(r)
        r0 = nr if r0 is None else r0
        ratios.append(nr / r0)
        if (ratios[-1] < tol) if strict else (ratios[-1] <= tol):
            return u, ratios, it
        ctx.dirichlet(list(bc_flags))
        ctx.schwarz_setup(1, combine)
        du, _, _ = ctx.gmres(-r, rtol=rtol, max_it=gmres_its, restart=restart, use_prec=True)
        u[own] += du
    raise RuntimeError("Newton did not reach %g: %r" % (tol, ratios))


NEWTON_CASES = [("p1_cube4", m) for m in hr.MODELS] + [("p2_cube2", m) for m in hr.MODELS]


def newton_mesh(lib, which):
    return lib.structured_mesh(3, 1, 4) if which == "p1_cube4" else mesh(lib, which)


EPS = 2.0 ** -52


@pytest.mark.parametrize("which,model", NEWTON_CASES)
def test_newton_at_abi_level_matches_the_host_loop(fedd_lib, ctx, which, model):
    """volume force -0.01 (E = 1, the reference's XML), Dirichlet on flag 2, GMRES to 1e-13, nonlinear residual ratio <= 1e-12.

    The ratio cannot be evaluated below one machine epsilon of the magnitudes its rows add up (hyperelastic_ref.
    residual_rounding_scale: the terms of the stress law, which cancel from the size of the moduli down to the size of the
    strain, through the quadrature and row sums), relative to |r_0|.  That floor follows from the inputs alone (it is taken at
    u = 0).  It lies below 1e-12 for every case but Mooney-Rivlin on the P2 cube, where C = 1 makes the brackets of the law
    three times larger than Neo-Hooke's and the floor is 1.6e-12 (the host loop stays at 1.1e-12 there): that case runs to its
    floor, every other one to the 1e-12 asked for; both facts are asserted."""
    m = newton_mesh(fedd_lib, which)
    params = PARAMS[model]
    ctx.mesh_set_dict(m)
    rhs = volume_rhs(fedd_lib, ctx, m, -0.01)
    is_dir = hr.dirichlet_mask(m)
    assert is_dir.any() and not is_dir.all()
    scale = hr.residual_rounding_scale(m, np.zeros_like(m["xyz"]), model, params)
    floor = EPS * np.linalg.norm(scale[~is_dir]) / np.linalg.norm(rhs[~is_dir])
    if (which, model) == ("p2_cube2", hr.MOONEY_RIVLIN):
        assert 1e-12 < floor < 2e-12, floor
    else:
        assert floor <= 1e-12, floor
    tol = max(1e-12, floor)
    u0, ratios0, its0 = hr.newton(m, model, params, rhs, is_dir, tol=tol)
    K0, _, _ = hr.assemble(m, u0.reshape(-1, 3)[m["gid_rep"]], model, params)
    import fedd_oracle as fo
    cond = np.linalg.cond(fo.set_dirichlet(K0, rhs, is_dir, 0.0)[0].toarray())
    assert cond * 1e-12 < 1e-8, cond            # what the two linear solves (direct; GMRES to 1e-13) can differ by stays below the bar
    u, ratios, its = gpu_newton(fedd_lib, ctx, m, model, params, rhs, tol=tol)
    print("%s %s: cond %.2e; floor %.2e; host %r; device %r" % (which, model, cond, floor, ratios0, ratios))
    assert its == its0 and its >= 3
    # superlinear decrease, the visible part of quadratic convergence: r_k+1 <= r_k^1.5 covers C r_k^2 with C <= r_k^-0.5.  It
    # can be seen only while r_k^2 lies above the accuracy the ratio can be evaluated to: steps from r_k >= 1e-6 are held to
    # the power (the first, from r_0 = 1, only to a decrease), later ones to the tolerance of the loop
    for r in (ratios, ratios0):
        for a, b in zip(r[:-1], r[1:]):
            assert b <= (a ** 1.5 if a >= 1e-6 else tol), r
    assert np.abs(u - u0).max() <= 1e-8 * np.abs(u0).max()

"""Surface load vectors and Neumann terms on the GPU (fedd_surface_set, fedd_assemble_surface[_values]) against a numpy
restatement of the surface integral: element loop, generic Gauss rules, bases from closed forms.  Every vector comparison
holds to 1e-10 x max|reference| (the project's parity bound); the measured maximum is printed in the assertion."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-10


# ---- numpy restatement: f_(i,d) = sum_S weight_S |S| / |ref| sum_q w_q phi_i(x_q) g_S[d], Gauss rules of 4 points per direction
# (exact to degree 7 on the line; on the triangle through the collapsed square, exact for the quadratic bases) ----
def gauss_rule(sdim):
    x, w = np.polynomial.legendre.leggauss(4)
    x, w = 0.5 * (x + 1), 0.5 * w
    if sdim == 1:
        return x[:, None], w
    u, v = np.meshgrid(x, x, indexing="ij")                     # (u, v) -> (u, v (1 - u)), Jacobian 1 - u
    return np.stack([u.ravel(), (v * (1 - u)).ravel()], axis=1), (np.outer(w, w) * (1 - u)).ravel()


def basis(sdim, nsn, p):
    x = p[:, 0]
    if sdim == 1:
        return np.stack([1 - x, x], 1) if nsn == 2 else np.stack([(1 - x) * (1 - 2 * x), x * (2 * x - 1), 4 * x * (1 - x)], 1)
    y = p[:, 1]
    l = 1 - x - y
    if nsn == 3:
        return np.stack([l, x, y], 1)
    return np.stack([l * (2 * l - 1), x * (2 * x - 1), y * (2 * y - 1), 4 * x * l, 4 * x * y, 4 * y * l], 1)


def surface_vector(xyz, surf, g_surf, weight=None):
    """xyz [n, dim], surf [ns, nsn], g_surf [ns, dofs] -> [n * dofs]"""
    dim, nsn, dofs = xyz.shape[1], surf.shape[1], g_surf.shape[1]
    pts, w = gauss_rule(dim - 1)
    base = w @ basis(dim - 1, nsn, pts)
    f = np.zeros((xyz.shape[0], dofs))
    for s, nodes in enumerate(surf):
        B = (xyz[nodes[1:dim]] - xyz[nodes[0]]).T
        scaling = np.linalg.norm(B[:, 0]) if dim == 2 else np.linalg.norm(np.cross(B[:, 0], B[:, 1]))
        f[nodes] += (1 if weight is None else weight[s]) * scaling * np.outer(base, g_surf[s])
    return f.ravel()


def measure(xyz, surf):
    d = xyz.shape[1]
    e1 = xyz[surf[:, 1]] - xyz[surf[:, 0]]
    return np.linalg.norm(e1, axis=1).sum() if d == 2 else 0.5 * np.linalg.norm(np.cross(e1, xyz[surf[:, 2]] - xyz[surf[:, 0]]), axis=1).sum()


def close(got, ref, what):
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    assert err <= TOL * scale, "%s: max deviation %.3e, bound %.3e" % (what, err, TOL * scale)


@pytest.fixture(scope="module")
def ctx(fedd_lib):
    c = fedd_lib.Context(device=0)
    yield c
    c.close()


_cache = {}


def file_mesh(fedd_lib, name, dim, p2):
    """(mesh dict, surface elements, flags), read and built once per module"""
    key = (name, p2)
    if key not in _cache:
        m = fedd_lib.read_mesh(os.path.join(GOLD, name), dim)
        if p2:
            _cache[key] = (fedd_lib.p2_of_p1(m, volume_id=int(np.bincount(m["elem_flag"]).argmax())), fedd_lib.p2_surfaces(m),
                           m["surf_flag"])
        else:
            _cache[key] = (m, m["surf"], m["surf_flag"])
    return _cache[key]


def upload(fedd_lib, c, m, surf, sflag, dofs):
    c.mesh_set_dict(m)
    c.pattern_build(dofs, fedd_lib.BLOCK_SCALAR if dofs == 1 else fedd_lib.BLOCK_DIAG)
    c.surface_set(surf, sflag)


@pytest.mark.parametrize("vector", [False, True])
@pytest.mark.parametrize("p2", [False, True])
@pytest.mark.parametrize("name,dim", [("square.mesh", 2), ("DFG3DCylinder_1k.mesh", 3)])
def test_per_flag_loads_and_boundary_measure(fedd_lib, ctx, name, dim, p2, vector):
    m, surf, sflag = file_mesh(fedd_lib, name, dim, p2)
    dofs = dim if vector else 1
    upload(fedd_lib, ctx, m, surf, sflag, dofs)
    flags = np.unique(sflag)
    g = np.array([[0.5 + 1.25 * k - 0.75 * d * (k + 1) for d in range(dofs)] for k in range(len(flags))])
    ctx.assemble_surface(g, flags=flags)
    got = ctx.rhs_get()
    ref = surface_vector(m["xyz"], surf, g[np.searchsorted(flags, sflag)])
    close(got, ref, "per-flag loads")
    # only some of the flags: the other elements contribute nothing
    ctx.assemble_surface(g[-1:], flags=flags[-1:])
    close(ctx.rhs_get(), surface_vector(m["xyz"], surf, g[-1][None, :] * (sflag == flags[-1])[:, None]), "one flag")
    # one load per surface element
    gs = g[np.searchsorted(flags, sflag)] * (1 + np.arange(len(sflag)) % 5)[:, None]
    ctx.assemble_surface_values(gs)
    close(ctx.rhs_get(), surface_vector(m["xyz"], surf, gs), "per-element loads")
    # g = 1 everywhere: the entries sum to the measure of the boundary, component by component
    ctx.assemble_surface(np.ones(dofs))
    total = ctx.rhs_get().reshape(-1, dofs).sum(axis=0)
    area = measure(m["xyz"], surf)
    if name == "square.mesh":
        assert abs(area - 4.0) <= 1e-12
    err = np.abs(total - area).max()
    assert err <= TOL * area, "sum of the vector %r, boundary measure %.15g" % (total, area)
    # a higher quadrature degree integrates the same polynomials
    ctx.assemble_surface(g, flags=flags, extra_degree=1)
    close(ctx.rhs_get(), ref, "extra degree 1")


def fan_mesh(n=300):
    """n tetrahedra around the axis from node 1 = (0,0,0) to node 0 = (0,0,1): the apex, node 0, holds n boundary triangles"""
    a = 2 * np.pi * np.arange(n) / n
    xyz = np.vstack([[0, 0, 1.0], [0, 0, 0.0], np.stack([np.cos(a), np.sin(a) * 1.5, 0.5 + 0.1 * np.cos(3 * a)], 1)])
    k = np.arange(n)
    conn = np.stack([np.zeros(n, int), np.ones(n, int), 2 + k, 2 + (k + 1) % n], 1).astype(np.int32)
    top = np.stack([np.zeros(n, int), 2 + k, 2 + (k + 1) % n], 1).astype(np.int32)
    gid = np.arange(n + 2, dtype=np.int64)
    return dict(dim=3, nen=4, conn=conn, xyz=xyz, gid_rep=gid, gid_uni=gid.copy(), flag_uni=np.zeros(n + 2, np.int32)), top


@pytest.mark.parametrize("n_surf", [0, 1, 63, 64, 65, 257])
def test_window_crossing_on_a_fan(fedd_lib, ctx, n_surf):
    """the apex' list of (surface element, local index) pairs crosses the wavefront width and the capacity of the LDS park"""
    m, top = fan_mesh()
    ctx.mesh_set_dict(m)
    ctx.pattern_build(3, fedd_lib.BLOCK_DIAG)
    surf = top[:n_surf]
    sflag = (1 + np.arange(n_surf) % 3).astype(np.int32)
    ctx.surface_set(surf.reshape(-1, 3), sflag)
    g = np.array([[1.0, -2.0, 0.25], [0.5, 3.0, -1.0], [-4.0, 0.125, 2.0]])
    before = np.random.default_rng(3).standard_normal(3 * (m["xyz"].shape[0]))
    if n_surf == 0:
        ctx.rhs_set(before)
        ctx.assemble_surface(g, flags=[1, 2, 3], accumulate=True)
        assert np.array_equal(ctx.rhs_get(), before), "accumulate = 1 on the empty set changed the right-hand side"
        ctx.assemble_surface(g, flags=[1, 2, 3], accumulate=False)
        assert not ctx.rhs_get().any(), "accumulate = 0 on the empty set left entries behind"
        return
    ref = surface_vector(m["xyz"], surf, g[sflag - 1])
    ctx.rhs_set(before)
    ctx.assemble_surface(g, flags=[1, 2, 3], accumulate=False)
    got = ctx.rhs_get()
    close(got, ref, "fan, %d surface elements" % n_surf)
    ctx.assemble_surface(g, flags=[1, 2, 3], accumulate=False)
    assert np.array_equal(ctx.rhs_get(), got), "two calls differ"
    # accumulating: untouched nodes keep their bits, touched ones get the host sum
    ctx.rhs_set(before)
    ctx.assemble_surface(g, flags=[1, 2, 3], accumulate=True)
    assert np.array_equal(ctx.rhs_get(), before + got)


def test_interior_face_counts_twice(fedd_lib, ctx):
    m = fedd_lib.structured_mesh(3, 1, 2)
    faces = {}
    for e in m["conn"]:
        for skip in range(4):
            faces.setdefault(tuple(sorted(np.delete(e, skip))), []).append(1)
    inner = np.array([k for k, v in sorted(faces.items()) if len(v) == 2][:5], dtype=np.int32)
    outer = np.array([k for k, v in sorted(faces.items()) if len(v) == 1][:3], dtype=np.int32)
    surf = np.vstack([inner, outer])
    ctx.mesh_set_dict(m)
    ctx.pattern_build(1, fedd_lib.BLOCK_SCALAR)
    ctx.surface_set(surf, np.full(len(surf), 7, np.int32))
    ctx.assemble_surface([1.5])
    w = np.array([2] * len(inner) + [1] * len(outer))
    close(ctx.rhs_get(), surface_vector(m["xyz"], surf, np.full((len(surf), 1), 1.5), weight=w), "interior faces")


def test_repeatable_and_accumulate_after_volume_load(fedd_lib, ctx):
    m = fedd_lib.structured_mesh(3, 1, 3)
    surf, sflag = fedd_lib.structured_surfaces(3, 1, 3)
    upload(fedd_lib, ctx, m, surf, sflag, 3)
    g = np.array([[1.0, 2.0, 3.0], [-1.0, 0.5, 0.25], [0.0, -3.0, 1.0]])
    ctx.assemble_surface(g, flags=[1, 2, 3])
    s1 = ctx.rhs_get()
    ctx.assemble_surface(g, flags=[1, 2, 3])
    s2 = ctx.rhs_get()
    assert np.array_equal(s1, s2), "two calls differ"
    ctx.assemble_rhs([0.3, -0.7, 1.1])
    v = ctx.rhs_get()
    ctx.assemble_surface(g, flags=[1, 2, 3], accumulate=True)
    assert np.array_equal(ctx.rhs_get(), v + s1), "accumulate = 1 is not the host sum of the two vectors"
    close(s1, surface_vector(m["xyz"], surf, g[sflag - 1]), "structured cube")


@pytest.mark.parametrize("layers", [1, 4])
def test_two_rank_meshes_without_communication(fedd_lib, layers):
    """the rank meshes of a 2 x 1 x 1 split of the 4^3-cell cube, each in its own context, one after the other: the owned rows
    placed by global id are the one-rank vector"""
    g = np.array([[1.0, 2.0, 3.0], [-1.0, 0.5, 0.25], [0.0, -3.0, 1.0]])
    m1 = fedd_lib.structured_mesh(3, 1, 4)
    s1, f1 = fedd_lib.structured_surfaces(3, 1, 4)
    ref = np.zeros(3 * m1["n_global"])
    ref.reshape(-1, 3)[m1["gid_rep"]] = surface_vector(m1["xyz"], s1, g[f1 - 1]).reshape(-1, 3)
    out = np.full((m1["n_global"], 3), np.nan)
    for rank in range(2):
        m = fedd_lib.structured_mesh(3, (2, 1, 1), [2, 4, 4], rank, ghosts=layers)
        surf, sflag = fedd_lib.structured_surfaces(3, (2, 1, 1), [2, 4, 4], rank, ghosts=layers)
        c = fedd_lib.Context(device=0)
        try:
            upload(fedd_lib, c, m, surf, sflag, 3)
            c.assemble_surface(g, flags=[1, 2, 3])
            out[m["gid_uni"]] = c.rhs_get().reshape(-1, 3)
        finally:
            c.close()
    assert not np.isnan(out).any()
    close(out.ravel(), ref, "two ranks, %d ghost layers" % layers)


def solve(fedd_lib, c):
    c.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
    x, its, rel = c.gmres(None, rtol=1e-12, max_it=400, restart=200, use_prec=True)
    assert rel <= 1e-12, "GMRES stopped at %.3e after %d iterations" % (rel, its)
    return x


def test_patch_laplace_flux(fedd_lib, ctx):
    """u = 0 on x = 0, flux g on x = 1, natural elsewhere: u = g x lies in the P1 space"""
    m = fedd_lib.structured_mesh(3, 1, 4)
    surf, sflag = fedd_lib.structured_surfaces(3, 1, 4)
    upload(fedd_lib, ctx, m, surf, sflag, 1)
    ctx.assemble(fedd_lib.FORM_LAPLACE)
    gflux = 0.75
    ctx.assemble_surface([gflux], flags=[3])
    ctx.dirichlet([2], [0.0])
    x = solve(fedd_lib, ctx)
    exact = gflux * m["xyz"][:, 0]
    err = np.abs(x - exact).max() / np.abs(exact).max()
    assert err <= 1e-9, "Laplace patch test: relative error %.3e" % err


def test_patch_elasticity_traction(fedd_lib, ctx):
    """traction (sigma, 0, 0) on x = 1, sliding supports on x = 0 (X), y = 0 (Y), z = 0 (Z): the uniaxial field"""
    m = fedd_lib.structured_mesh(3, 1, 4)
    surf, sflag = fedd_lib.structured_surfaces(3, 1, 4)
    ctx.mesh_set_dict(m)
    ctx.pattern_build(3, fedd_lib.BLOCK_FULL)
    ctx.surface_set(surf, sflag)
    mu, nu, sigma = 1.0, 0.3, 0.2
    lam = 2.0 * mu * nu / (1.0 - 2.0 * nu)
    E = mu * (3 * lam + 2 * mu) / (lam + mu)
    ctx.assemble(fedd_lib.FORM_LINELAS, [lam, mu])
    ctx.assemble_surface([[sigma, 0.0, 0.0]], flags=[3])
    mask = (np.abs(m["xyz"]) < 1e-12).astype(np.int32)        # component d is held on the plane x_d = 0
    nodes = np.nonzero(mask.any(axis=1))[0].astype(np.int32)
    ctx.dirichlet_nodes(nodes, np.zeros((len(nodes), 3)), comp_mask=mask[nodes])
    x = solve(fedd_lib, ctx).reshape(-1, 3)
    exact = m["xyz"] * np.array([sigma / E, -nu * sigma / E, -nu * sigma / E])
    err = np.abs(x - exact).max() / np.abs(exact).max()
    assert err <= 1e-9, "elasticity patch test: relative error %.3e" % err


def test_errors(fedd_lib, ctx):
    m = fedd_lib.structured_mesh(3, 1, 2)
    surf, sflag = fedd_lib.structured_surfaces(3, 1, 2)
    ctx.mesh_set_dict(m)
    ctx.pattern_build(1, fedd_lib.BLOCK_SCALAR)
    with pytest.raises(fedd_lib.FeddError, match="fedd_surface_set first"):     # fedd_mesh_set dropped the earlier set
        ctx.assemble_surface([1.0])
    with pytest.raises(fedd_lib.FeddError, match="out of range"):
        ctx.surface_set(surf + 1000, sflag)
    with pytest.raises(fedd_lib.FeddError, match="nodes, not 4"):
        ctx.surface_set(np.zeros((2, 4), np.int32), sflag[:2])
    ctx.surface_set(surf, sflag)
    with pytest.raises(fedd_lib.FeddError, match="up to degree|not on the hot path"):
        ctx.assemble_surface([1.0], extra_degree=9)

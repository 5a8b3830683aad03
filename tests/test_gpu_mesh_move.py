"""fedd_mesh_move on the GPU: a context whose mesh was moved computes, bit for bit, what a fresh context computes that was given
x_ref + d through fedd_mesh_set (x_ref + d formed in numpy: the same single addition), and the move runs nothing of the symbolic
stage again.

Four meshes, the smallest that reach each kernel family:
  cube_p1    3D P1, 4^3 cells    tile path at the default dispatch, and the pair sweep ("asm_kind" 2)
  square_p1  2D P1, 5 x 5
  channel_p2 2D P2 / P1, 4 x 4   fedd_assemble_div, fedd_assemble_advection (N, N + W), fedd_assemble_stress
  cube_p2    3D P2, 2^3 cells    fedd_assemble_hyperelastic (tangent and force)
The displacement is smooth, 0.2 h (sin, cos products), and exactly zero on the boundary; numpy shows here that it keeps every
|det B| / |det B_ref| above 0.3, and the device's min_det_ratio must agree with that number to 1e-12 relative (both evaluate the
same expansion of the determinant; the two differ by the rounding of a handful of products).
The solver tests take a larger amplitude (0.6 h, ratios above 0.5) so that nodes change their Schwarz box, which numpy asserts by the binning
rule of include/fedd_hip.h: a stale box lattice would give other subdomains than the fresh context's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = {"cube_p1": (3, 4, False), "square_p1": (2, 5, False), "channel_p2": (2, 4, True), "cube_p2": (3, 2, True)}
LAME = [1.5, 0.8]
NEOHOOKE = [3.0e3, 0.4]
_meshes, _fresh = {}, {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def mesh(lib, case):
    if case not in _meshes:
        dim, M, p2 = CASES[case]
        m = lib.structured_mesh(dim, 1, M)
        m["surf"], m["surf_flag"] = lib.structured_surfaces(dim, 1, M)
        if p2:
            s2 = lib.p2_surfaces(m)
            sflag = m["surf_flag"]
            m = lib.p2_of_p1(m, volume_id=0)
            m["surf"], m["surf_flag"] = s2, sflag
        m["h"] = 1.0 / M
        _meshes[case] = m
    return _meshes[case]


def displacement(m, amp=0.2, phase=0.0):
    """amp * h * (sin, cos products) in every component, exactly zero on the boundary of the unit square / cube"""
    x = m["xyz"]
    dim = m["dim"]
    bubble = np.prod(np.sin(np.pi * x), axis=1)
    cols = [bubble * np.cos(2.1 * x[:, (k + 1) % dim] + 0.7 * k + phase) * np.sin(1.7 * x[:, k] + 1.1 + phase) for k in range(dim)]
    d = amp * m["h"] * np.stack(cols, axis=1)
    d[np.any((x == 0.0) | (x == 1.0), axis=1)] = 0.0
    return d


def det_b(m, x):
    """det B of every element from its first dim + 1 nodes, in the expansion of the device (assemble_common.hpp affine_det)"""
    dim = m["dim"]
    X = x[m["conn"][:, :dim + 1]]
    B = np.transpose(X[:, 1:] - X[:, :1], (0, 2, 1))       # B[e][i][j] = x_{j+1}[i] - x_0[i]
    if dim == 2:
        return B[:, 0, 0] * B[:, 1, 1] - B[:, 1, 0] * B[:, 0, 1]
    return (B[:, 0, 0] * B[:, 1, 1] * B[:, 2, 2] + B[:, 0, 1] * B[:, 1, 2] * B[:, 2, 0] + B[:, 0, 2] * B[:, 1, 0] * B[:, 2, 1] -
            B[:, 2, 0] * B[:, 1, 1] * B[:, 0, 2] - B[:, 2, 1] * B[:, 1, 2] * B[:, 0, 0] - B[:, 2, 2] * B[:, 1, 0] * B[:, 0, 1])


def min_ratio(m, d):
    r = det_b(m, m["xyz"] + d) / det_b(m, m["xyz"])
    return float(np.min(r))


def moved(m, d):
    out = dict(m)
    out["xyz"] = m["xyz"] + d       # the single addition of Mesh::moveMesh
    return out


def velocity(m):
    x = m["xyz"]
    s = x.sum(axis=1)
    cols = [np.sin(1.3 * x[:, 0] + 0.4 * s) + 0.5, np.cos(0.9 * x[:, 1] - 0.7 * s) * np.exp(0.3 * x[:, 0])]
    if m["dim"] == 3:
        cols.append(np.sin(1.1 * x[:, 2]) * np.cos(0.8 * s) - 0.25)
    return np.stack(cols, axis=1)


def csr(c):
    rp, col, val, _ = c.csr_get()
    return {"indptr": rp, "indices": col, "values": val}


def slot(c, k):
    A = c.matrix_get(k)
    return {"indptr": A.indptr.copy(), "indices": A.indices.copy(), "values": A.data.copy()}


def flat(prefix, d):
    return {prefix + "." + k: v for k, v in d.items()}


# ---- the groups of calls: each returns {name: array}.  m gives sizes and the velocity only (the REFERENCE coordinates on
#      both sides: the field does not move with the mesh).  setup = False leaves out fedd_surface_set and fedd_velocity_set:
#      the run after a move uses the surface set and the velocity that were given before it ----
def g_scalar(lib, c, m, setup=True):
    out = {}
    c.pattern_build(1, lib.BLOCK_SCALAR)
    c.assemble(lib.FORM_LAPLACE)
    out.update(flat("laplace", csr(c)))
    c.assemble(lib.FORM_MASS)
    out.update(flat("mass", csr(c)))
    c.assemble_rhs([1.3])
    out["rhs"] = c.rhs_get()
    if setup:
        c.surface_set(m["surf"], m["surf_flag"])
    c.assemble_surface([0.7])
    out["surface"] = c.rhs_get()
    return out


def g_vector(lib, c, m, setup=True):
    dim = m["dim"]
    out = {}
    c.pattern_build(dim, lib.BLOCK_FULL)
    c.assemble(lib.FORM_LINELAS, LAME)
    out.update(flat("elasticity", csr(c)))
    c.assemble_rhs([1.0, -2.0, 0.5][:dim])
    out["rhs_vec"] = c.rhs_get()
    if setup:
        c.surface_set(m["surf"], m["surf_flag"])
    c.assemble_surface([0.3, -0.4, 0.9][:dim])
    out["surface_vec"] = c.rhs_get()
    return out


def g_scalar_k2(lib, c, m, setup=True):         # under option "asm_kind" 2 (OPTIONS below): the pair sweep instead of the tiles
    return {"k2." + k: v for k, v in g_scalar(lib, c, m, setup).items()}


def g_vector_k2(lib, c, m, setup=True):
    return {"k2." + k: v for k, v in g_vector(lib, c, m, setup).items()}


def g_flow(lib, c, m, setup=True):
    out = {}
    c.assemble_div(m["n_p1"], 1, 2)
    out.update(flat("B", slot(c, 1)))
    out.update(flat("BT", slot(c, 2)))
    if setup:
        c.velocity_set(velocity(m))
    c.assemble_advection(lib.ADV_N, 1.0, -1, 4)
    out.update(flat("N", slot(c, 4)))
    c.assemble_advection(lib.ADV_NEWTON, 1.0, -1, 4)
    out.update(flat("NW", slot(c, 4)))
    return out


def g_stress(lib, c, m, setup=True):
    c.pattern_build(m["dim"], lib.BLOCK_FULL)
    c.assemble_stress()
    return flat("stress", csr(c))


def g_hyper(lib, c, m, setup=True):
    c.pattern_build(m["dim"], lib.BLOCK_FULL)
    if setup:
        c.velocity_set(0.02 * velocity(m))
    c.assemble_hyperelastic(lib.HYPER_NEOHOOKE, NEOHOOKE)
    out = flat("tangent", csr(c))
    out["force"] = c.hyperelastic_force_get()
    return out


GROUPS = {"cube_p1": (g_scalar, g_vector, g_scalar_k2, g_vector_k2), "square_p1": (g_scalar, g_vector),
          "channel_p2": (g_scalar, g_vector, g_flow, g_stress), "cube_p2": (g_scalar, g_vector, g_hyper)}
OPTIONS = {g_scalar_k2: ("asm_kind", 2), g_vector_k2: ("asm_kind", 2)}      # set around the whole group, its warm-up included


def with_option(c, g, on):
    if g in OPTIONS:
        c.set_option(OPTIONS[g][0], OPTIONS[g][1] if on else 0)


def fresh(lib, case, key, d):
    """every group of the case on a fresh context that was given x_ref + d; computed once per (case, displacement)"""
    if (case, key) not in _fresh:
        m = mesh(lib, case)
        c = lib.Context(device=0)
        try:
            c.mesh_set_dict(moved(m, d))
            out = {}
            for g in GROUPS[case]:
                with_option(c, g, True)
                out[g.__name__] = g(lib, c, m)
                with_option(c, g, False)
        finally:
            c.close()
        _fresh[(case, key)] = out
    return _fresh[(case, key)]


def assert_same(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        a, b = got[k], want[k]
        if a.dtype == np.float64:
            n = int(np.count_nonzero(bits(a) != bits(b))) if a.shape == b.shape else -1
            assert n == 0, "%s: %s differs from the fresh context in %d entries" % (what, k, n)
        else:
            assert np.array_equal(a, b), "%s: %s differs from the fresh context" % (what, k)


def counters(c):
    return c.timing_get()["symbolic"][1], c.mesh_setup_info(), c.pattern_reuse_info()["n_reused"]


@pytest.fixture()
def ctx(fedd_lib):
    c = fedd_lib.Context(device=0)
    yield c
    c.close()


@pytest.mark.parametrize("case", list(CASES))
def test_moved_context_equals_fresh_context_bit_for_bit(fedd_lib, ctx, case):
    lib = fedd_lib
    m = mesh(lib, case)
    d = displacement(m)
    assert np.abs(d).max() > 0.05 * m["h"] and not d[np.any((m["xyz"] == 0.0) | (m["xyz"] == 1.0), axis=1)].any()
    r_np = min_ratio(m, d)
    print(case, "numpy min det ratio %.6f" % r_np)
    assert r_np > 0.3           # the fixture is nowhere near an inversion
    want = fresh(lib, case, "d", d)
    ctx.timing_enable(True)
    ctx.mesh_set_dict(m)
    for g in GROUPS[case]:
        with_option(ctx, g, True)
        ctx.mesh_move(None)
        g(lib, ctx, m)                      # on the reference coordinates: every per-mesh structure of the group now exists
        before = counters(ctx)
        id0 = ctx.mesh_move_info()["geometry_id"]
        ctx.mesh_move(d)
        info = ctx.mesh_move_info()
        assert info["geometry_id"] == id0 + 1
        assert abs(info["min_det_ratio"] - r_np) <= 1e-12 * r_np, (info["min_det_ratio"], r_np)
        assert np.array_equal(bits(ctx.mesh_coords()), bits(m["xyz"] + d))
        assert counters(ctx) == before      # the move itself
        got = g(lib, ctx, m, setup=False)   # the surface set and the velocity of before the move
        with_option(ctx, g, False)
        assert_same(got, want[g.__name__], case + " " + g.__name__)
        after = counters(ctx)
        print(case, g.__name__, "symbolic launches, mesh setup, patterns kept: before", before, "after", after)
        assert after[0] == before[0], "the symbolic stage ran again after a move"
        assert after[1] == before[1]
        if g is not g_flow:                 # (fedd_assemble_div asks for no fedd_pattern_build)
            assert after[2] > before[2], "the pattern build after a move did not repeat"
    if case == "cube_p1":
        assert ctx.mesh_setup_info()["tiles_state"] == 1, "the 4^3 cube is meant to take the tile path"


@pytest.mark.parametrize("case", ["cube_p1", "channel_p2"])
def test_moves_are_relative_to_the_uploaded_coordinates(fedd_lib, ctx, case):
    lib = fedd_lib
    m = mesh(lib, case)
    d1, d2 = displacement(m, 0.2, phase=0.9), displacement(m)
    want = fresh(lib, case, "d", d2)["g_scalar"]
    ctx.mesh_set_dict(m)
    at_ref = g_scalar(lib, ctx, m)
    ctx.mesh_move(d1)
    after_d1 = g_scalar(lib, ctx, m)
    assert not np.array_equal(bits(after_d1["laplace.values"]), bits(at_ref["laplace.values"]))
    ctx.mesh_move(d2)                       # not d1 + d2
    assert_same(g_scalar(lib, ctx, m), want, case + " after move(d1), move(d2)")
    ctx.mesh_move(None)
    assert np.array_equal(bits(ctx.mesh_coords()), bits(m["xyz"]))
    assert_same(g_scalar(lib, ctx, m), at_ref, case + " after move(NULL)")
    info = ctx.mesh_move_info()
    assert (info["n_moves"], info["min_det_ratio"]) == (3, 1.0)
    ctx.mesh_set_dict(m)                    # a new reference: the count of its moves starts again, geometry_id goes on
    assert ctx.mesh_move_info()["n_moves"] == 0 and ctx.mesh_move_info()["geometry_id"] == info["geometry_id"]


# ---- solver after a move ----
def schwarz_boxes(x_own, target, scale=1.0):
    """box of every owned node under the rule of fedd_schwarz_setup (include/fedd_hip.h): a lattice over the bounding box of
    the owned nodes, edge s = scale (V target / n)^(1/dim), an odd number g = ceil(L / s) of boxes per direction of width
    w = L / g, node -> floor((x - lo) / w) (a node within 1e-9 w of a box boundary goes to the box on the centre side)"""
    n, dim = x_own.shape
    lo, hi = x_own.min(axis=0), x_own.max(axis=0)
    L = hi - lo
    s = scale * (np.prod(L) * target / n) ** (1.0 / dim)
    box = np.zeros(n, dtype=np.int64)
    mul = 1
    for k in range(dim):
        g = int(np.ceil(L[k] / s - 1e-9))
        g = max(g, 1)
        g += 1 - g % 2
        t = (x_own[:, k] - lo[k]) / (L[k] / g)
        kb = np.floor(t + 0.5)
        ix = np.floor(t)
        tie = np.abs(t - kb) <= 1e-9
        ix[tie] = np.where(2 * kb[tie] <= g - 1, kb[tie], kb[tie] - 1)
        box += mul * np.clip(ix, 0, g - 1).astype(np.int64)
        mul *= g
    return box


def solve(lib, c, m, case, two_level, target, scale):
    """assemble, Dirichlet, Schwarz setup, GMRES; returns what the two contexts must agree on"""
    dim = m["dim"]
    if case == "cube_p1":
        c.pattern_build(1, lib.BLOCK_SCALAR)
        c.assemble(lib.FORM_LAPLACE)
        c.assemble_rhs([1.0])
    else:                                   # the velocity space of the channel: elasticity, two dofs per P2 node
        c.pattern_build(dim, lib.BLOCK_FULL)
        c.assemble(lib.FORM_LINELAS, LAME)
        c.assemble_rhs([1.0, -0.5])
    c.dirichlet(sorted(set(int(f) for f in m["flag_uni"]) - {0, 10}))
    c.schwarz_set_target(target, scale)
    c.schwarz_setup(1, lib.COMBINE_RESTRICTED, 1 if two_level else 0, lib.COARSE_Q1 if two_level else 0)
    info = c.schwarz_info()
    sizes = (info["sum_sizes"], info["sum_owned"])
    coarse = None
    if two_level:
        g, n0 = c.schwarz_coarse_sizes()
        coarse = (tuple(int(v) for v in g), n0)
    x, its, rel = c.gmres(rtol=1e-11, max_it=200, restart=200)
    assert rel <= 1e-11
    return {"info": info, "sizes": sizes, "coarse": coarse, "its": its, "x": x}


@pytest.mark.parametrize("two_level", [False, True])
@pytest.mark.parametrize("case", ["cube_p1", "channel_p2"])
def test_solver_after_a_move(fedd_lib, ctx, case, two_level):
    lib = fedd_lib
    m = mesh(lib, case)
    # 5 boxes of width 0.2 per direction, on the cube's 5^3 lattice (target 8 nodes at scale 0.6: edge 0.24) and on the channel's
    # 9 x 9 lattice (target 4: edge 0.22): the nodes next to a box boundary are 0.05 / 0.025 away from it
    target, scale = (8, 0.6) if case == "cube_p1" else (4, 1.0)
    d = displacement(m, 0.6)
    r_np = min_ratio(m, d)
    assert r_np > 0.3
    own = np.searchsorted(m["gid_rep"], m["gid_uni"])      # (one rank: the two maps hold the same nodes)
    assert np.array_equal(m["gid_rep"][own], m["gid_uni"])
    b0, b1 = schwarz_boxes(m["xyz"][own], target, scale), schwarz_boxes((m["xyz"] + d)[own], target, scale)
    changed = int(np.count_nonzero(b0 != b1))
    print(case, "two-level" if two_level else "one-level", "nodes that change their box:", changed, "min det ratio %.4f" % r_np)
    assert changed >= 1
    f = lib.Context(device=0)
    try:
        f.mesh_set_dict(moved(m, d))
        want = solve(lib, f, m, case, two_level, target, scale)
    finally:
        f.close()
    ctx.mesh_set_dict(m)
    at_ref = solve(lib, ctx, m, case, two_level, target, scale)                  # a box structure of the reference coordinates exists
    ctx.mesh_move(d)
    with pytest.raises(lib.FeddError):      # the preconditioner went with the coordinates it was laid over
        ctx.schwarz_apply(np.ones(ctx.csr_sizes()[0]))
    got = solve(lib, ctx, m, case, two_level, target, scale)
    assert not ctx.schwarz_reuse_info()["last_reused"]
    assert got["info"] == want["info"] and got["sizes"] == want["sizes"] and got["coarse"] == want["coarse"]
    assert got["its"] == want["its"]
    err = np.linalg.norm(got["x"] - want["x"]) / np.linalg.norm(want["x"])
    print("iterations", got["its"], "(reference coordinates: %d)" % at_ref["its"], "relative difference of the solutions %.2e" % err)
    assert err <= 1e-10


# ---- inversion ----
def test_an_inverting_move_is_refused_and_commits_nothing(fedd_lib, ctx):
    lib = fedd_lib
    m = mesh(lib, "cube_p1")
    ctx.mesh_set_dict(m)
    d_ok = displacement(m)
    ctx.mesh_move(d_ok)
    before = g_scalar(lib, ctx, m)
    info0, x0 = ctx.mesh_move_info(), ctx.mesh_coords()
    # the centre vertex through the face opposite to it in its elements: more than one cell width along x
    centre = int(np.argmin(np.linalg.norm(m["xyz"] - 0.5, axis=1)))
    bad = d_ok.copy()
    bad[centre, 0] += 1.6 * m["h"]
    r = det_b(m, m["xyz"] + bad) / det_b(m, m["xyz"])
    inverted = np.flatnonzero(r <= 0.0)
    assert inverted.size >= 1
    with pytest.raises(lib.FeddError, match=r"element (\d+) is inverted") as e:
        ctx.mesh_move(bad)
    named = int(__import__("re").search(r"element (\d+) is inverted", str(e.value)).group(1))
    print("refused:", e.value)
    assert named == int(inverted.min()) and ("%.6g" % r[named]) in str(e.value)
    assert ctx.mesh_move_info() == info0
    assert np.array_equal(bits(ctx.mesh_coords()), bits(x0))
    assert_same(g_scalar(lib, ctx, m), before, "after a refused move")
    ctx.mesh_move(d_ok)                     # and the context goes on working
    assert ctx.mesh_move_info()["n_moves"] == info0["n_moves"] + 1


# ---- stored slots and histories ----
def test_slots_and_histories_survive_and_the_combine_is_not_current(fedd_lib, ctx):
    lib = fedd_lib
    m = mesh(lib, "square_p1")
    dim = m["dim"]
    ctx.mesh_set_dict(m)
    ctx.pattern_build(dim, lib.BLOCK_DIAG)
    ctx.assemble(lib.FORM_MASS_VEC)
    ctx.matrix_store(5)
    ctx.assemble(lib.FORM_LAPLACE_VEC)
    ctx.matrix_store(0)
    ctx.matrix_combine(5, 2.0, 0, 1.0)
    assert ctx.matrix_combine_current(5, 2.0, 0, 1.0)
    M0, A0 = slot(ctx, 5), slot(ctx, 0)
    n = ctx.csr_sizes()[0]
    rng = np.random.default_rng(5)
    u0, u1 = rng.standard_normal(n), rng.standard_normal(n)
    ctx.multistep_begin(2)
    ctx.solution_set(u0)
    ctx.multistep_advance(5, [1.0 / 0.1])
    ctx.solution_set(u1)
    ctx.multistep_advance(5, [1.5 / 0.1, -2.0 / 0.1])
    id0 = ctx.mesh_move_info()["geometry_id"]
    ctx.mesh_move(displacement(m))
    assert ctx.mesh_move_info()["geometry_id"] == id0 + 1          # how a caller tells that the slots are of another geometry
    assert not ctx.matrix_combine_current(5, 2.0, 0, 1.0)
    assert_same(slot(ctx, 5), M0, "slot 5 after the move")
    assert_same(slot(ctx, 0), A0, "slot 0 after the move")
    assert ctx.multistep_info() == (2, 2)
    assert np.array_equal(bits(ctx.multistep_get(0)), bits(u1)) and np.array_equal(bits(ctx.multistep_get(1)), bits(u0))
    ctx.solution_set(u0)
    ctx.multistep_advance(5, [1.5 / 0.1, -2.0 / 0.1])             # ... and the loop goes on


def test_errors(fedd_lib, ctx):
    with pytest.raises(fedd_lib.FeddError, match="fedd_mesh_set first"):
        ctx.mesh_move(None)
    two = fedd_lib.Context(device=0, rank=0, nranks=2)      # (no communicator: the rank count alone decides)
    try:
        m = mesh(fedd_lib, "square_p1")
        two.mesh_set_dict(m)
        with pytest.raises(fedd_lib.FeddError, match="one rank"):
            two.mesh_move(np.zeros_like(m["xyz"]))
    finally:
        two.close()

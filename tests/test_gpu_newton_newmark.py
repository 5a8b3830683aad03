"""Nonlinear Newmark at the ABI level (include/fedd_hip.h "Nonlinear Newmark"; hyperelastic.hip, newton.hip):

  1  the fused time tangent fedd_assemble_hyperelastic_time against the public sequence it replaces, bit for bit
  2  fedd_newton_residual against the numpy restatement of the header's operation order built from public pieces, bit for bit
  3  the state: begin / update / end, and the errors
  4  one Newmark-Newton step, device-resident against the same step with the existing entries and host vectors
  5  the small-amplitude limit against the linear Newmark path (the restatement's own ratio is checked first)

References are computed once per module and shared."""
import os

import numpy as np
import pytest

import fedd_oracle as fo
import hyperelastic_ref as hr
from test_gpu_hyperelastic import PARAMS, mesh, model_id, own_dofs, smooth_displacement

pytestmark = pytest.mark.gpu

DT1, BETA, GAMMA = 0.01, 0.25, 0.5
CM1 = 1.0 / ((DT1 * DT1) * BETA)        # the coefficient of fedd_newmark_advance, evaluated as the header writes it
SLOT_MD, SLOT_A, SLOT_MF, SLOT_FREE, SLOT_EMPTY = 0, 1, 2, 3, 5
EPS = 2.0 ** -52


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture()
def ctx(fedd_lib):
    c = fedd_lib.Context(device=0)
    yield c
    c.close()


_meshes = {}


def get_mesh(lib, which):
    if which not in _meshes:
        if which == "p1_cube4":
            _meshes[which] = lib.structured_mesh(3, 1, 4)
        elif which == "p1_square6":
            _meshes[which] = lib.structured_mesh(2, 1, 6)
        else:
            _meshes[which] = mesh(lib, which)
    return _meshes[which]


def setup_masses(lib, ctx, m, density=1.0):
    """slot 0: density * vector mass on the DIAG pattern; slot 1: linear elasticity (FULL); slot 2: the same mass on the FULL
    pattern (the combine 1.0 * M + 0.0 * A); the system is left with the FULL pattern"""
    dim = m["dim"]
    ctx.mesh_set_dict(m)
    ctx.pattern_build(dim, lib.BLOCK_DIAG)
    ctx.assemble(lib.FORM_MASS_VEC)
    ctx.matrix_store(SLOT_MD)
    if density != 1.0:
        ctx.matrix_scale(SLOT_MD, density)
    ctx.pattern_build(dim, lib.BLOCK_FULL)
    ctx.assemble(lib.FORM_LINELAS, list(hr.stvk_params(0.3571, 0.4)))
    ctx.matrix_store(SLOT_A)
    ctx.matrix_combine(SLOT_MD, 1.0, SLOT_A, 0.0)
    ctx.matrix_store(SLOT_MF)


def set_u(ctx, m, u_glob):
    ctx.velocity_set(np.asarray(u_glob).reshape(-1, m["dim"])[m["gid_rep"]])


# ---------------------------------------------------------------------------------------------------------------------------
# 1  fused tangent = assemble -> store -> combine
# ---------------------------------------------------------------------------------------------------------------------------
FUSED_CASES = [("p1_square6", hr.STVK), ("p1_cube4", hr.NEOHOOKE), ("p1_cube4", hr.MOONEY_RIVLIN), ("p2_cube2", hr.NEOHOOKE)]


@pytest.mark.parametrize("which,model", FUSED_CASES)
@pytest.mark.parametrize("slot_m", [SLOT_MD, SLOT_MF], ids=["diag_mass", "full_mass"])
def test_fused_tangent_equals_store_and_combine(fedd_lib, ctx, which, model, slot_m):
    lib = fedd_lib
    m = get_mesh(lib, which)
    setup_masses(lib, ctx, m, density=1.7)
    u = smooth_displacement(m)
    mid, p = model_id(lib, model), PARAMS[model]
    set_u(ctx, m, u)
    ctx.assemble_hyperelastic(mid, p, lib.HYPER_TANGENT | lib.HYPER_FORCE)
    f_seq = ctx.hyperelastic_force_get()
    ctx.matrix_store(SLOT_FREE)
    ctx.matrix_combine(slot_m, CM1, SLOT_FREE, 1.0)
    rp_seq, ci_seq, v_seq, _ = ctx.csr_get()
    assert np.abs(v_seq).max() > 0.0

    def scribble():         # other values in the system matrix and the force vector in between
        set_u(ctx, m, 0.5 * u)
        ctx.assemble_hyperelastic(mid, p)
        set_u(ctx, m, u)

    scribble()
    ctx.assemble_hyperelastic_time(mid, p, slot_m, CM1)
    rp, ci, v, _ = ctx.csr_get()
    assert np.array_equal(rp, rp_seq) and np.array_equal(ci, ci_seq)
    assert np.array_equal(bits(v), bits(v_seq))
    assert np.array_equal(bits(ctx.hyperelastic_force_get()), bits(f_seq))
    # the mass term is in: the tangent alone differs
    ctx.assemble_hyperelastic(mid, p, lib.HYPER_TANGENT)
    assert not np.array_equal(ctx.csr_get()[2], v_seq)
    # tangent-only and force-only calls give the bits of the combined call
    scribble()
    ctx.assemble_hyperelastic_time(mid, p, slot_m, CM1, what=lib.HYPER_TANGENT)
    assert np.array_equal(bits(ctx.csr_get()[2]), bits(v_seq))
    scribble()
    before = ctx.csr_get()[2]
    ctx.assemble_hyperelastic_time(mid, p, slot_m, CM1, what=lib.HYPER_FORCE)
    assert np.array_equal(bits(ctx.hyperelastic_force_get()), bits(f_seq))
    assert np.array_equal(bits(ctx.csr_get()[2]), bits(before))         # a force-only call leaves the matrix alone


def test_fused_tangent_inverted_element_leaves_matrix_and_force(fedd_lib, ctx):
    lib = fedd_lib
    m = get_mesh(lib, "p1_cube4")
    setup_masses(lib, ctx, m)
    x = np.zeros((int(m["n_global"]), 3))
    x[m["gid_rep"]] = m["xyz"]
    mid, p = lib.HYPER_NEOHOOKE, PARAMS[hr.NEOHOOKE]
    set_u(ctx, m, smooth_displacement(m))
    ctx.assemble_hyperelastic_time(mid, p, SLOT_MD, CM1)
    v0, f0 = ctx.csr_get()[2], ctx.hyperelastic_force_get()
    set_u(ctx, m, -2.0 * x)                      # F = -I everywhere: the first inverted element is 0
    with pytest.raises(lib.FeddError, match=r"fedd_assemble_hyperelastic_time: element 0 is inverted"):
        ctx.assemble_hyperelastic_time(mid, p, SLOT_MD, CM1)
    assert np.array_equal(bits(ctx.csr_get()[2]), bits(v0))
    assert np.array_equal(bits(ctx.hyperelastic_force_get()), bits(f0))


def test_fused_tangent_errors(fedd_lib, ctx):
    lib = fedd_lib
    m = get_mesh(lib, "p1_cube4")
    setup_masses(lib, ctx, m)
    ctx.pattern_build(1, lib.BLOCK_SCALAR)
    ctx.assemble(lib.FORM_MASS)
    ctx.matrix_store(4)                          # a scalar mass: another space
    ctx.pattern_build(3, lib.BLOCK_FULL)
    set_u(ctx, m, smooth_displacement(m))
    nh = (lib.HYPER_NEOHOOKE, PARAMS[hr.NEOHOOKE])
    with pytest.raises(lib.FeddError, match="slot %d is empty" % SLOT_EMPTY):
        ctx.assemble_hyperelastic_time(*nh, SLOT_EMPTY, CM1)
    with pytest.raises(lib.FeddError, match="out of range"):
        ctx.assemble_hyperelastic_time(*nh, 7, CM1)
    with pytest.raises(lib.FeddError, match="one space"):
        ctx.assemble_hyperelastic_time(*nh, 4, CM1)
    ctx.pattern_build(3, lib.BLOCK_DIAG)
    with pytest.raises(lib.FeddError, match="FULL pattern"):
        ctx.assemble_hyperelastic_time(*nh, SLOT_MD, CM1)
    ctx.mesh_set_dict(m)                         # the slots now belong to an earlier mesh
    ctx.pattern_build(3, lib.BLOCK_FULL)
    set_u(ctx, m, smooth_displacement(m))
    with pytest.raises(lib.FeddError, match="current mesh"):
        ctx.assemble_hyperelastic_time(*nh, SLOT_MD, CM1)


# ---------------------------------------------------------------------------------------------------------------------------
# 2  the residual restated from public pieces
# ---------------------------------------------------------------------------------------------------------------------------
def flagged_rows(m, flag, comps):
    """owned rows of the nodes with that flag, components comps"""
    dim = m["dim"]
    nodes = np.nonzero(np.asarray(m["flag_uni"]) == flag)[0]
    return (dim * nodes[:, None] + np.asarray(comps)[None, :]).ravel()


@pytest.mark.parametrize("which,model", [("p1_cube4", hr.NEOHOOKE), ("p1_square6", hr.STVK)])
@pytest.mark.parametrize("slot_m", [SLOT_MD, SLOT_MF], ids=["diag_mass", "full_mass"])
@pytest.mark.parametrize("with_source", [False, True], ids=["no_source", "source"])
def test_residual_equals_the_restatement_bit_for_bit(fedd_lib, ctx, which, model, slot_m, with_source):
    lib = fedd_lib
    m = get_mesh(lib, which)
    dim = m["dim"]
    setup_masses(lib, ctx, m, density=1.3)
    own = own_dofs(m)
    n = own.shape[0]
    rng = np.random.default_rng(5)
    u = smooth_displacement(m).ravel()[own]
    b = rng.uniform(-1.0, 1.0, n)
    s = rng.uniform(-1.0, 1.0, n)
    g = 0.37
    comp = 1
    mask = [1 if d == comp else 0 for d in range(dim)]
    rows = flagged_rows(m, 2, [comp])
    assert 0 < rows.shape[0] < n // dim
    ctx.solution_set(u)
    ctx.rhs_set(b)
    ctx.newton_begin()
    if with_source:
        ctx.newton_source_set(s)
    assert ctx.newton_info()["have_source"] == with_source
    ctx.assemble_hyperelastic(model_id(lib, model), PARAMS[model], lib.HYPER_FORCE)      # u is the nodal field begin wrote
    f = ctx.hyperelastic_force_get()
    ug = np.zeros(dim * int(m["n_global"]))
    ug[own] = u
    _, f_ref, _ = hr.assemble(m, ug.reshape(-1, dim)[m["gid_rep"]], model, PARAMS[model])
    assert np.abs(f - f_ref[own]).max() <= 1e-10 * np.abs(f_ref).max()                  # begin put u_k where the assembly reads it
    nr1 = ctx.newton_residual(slot_m, CM1, [2], values=[g] * dim, comp_mask=mask)
    r1 = ctx.rhs_get()
    nr2 = ctx.newton_residual(slot_m, CM1, [2], values=[g] * dim, comp_mask=mask)
    r2 = ctx.rhs_get()
    # the restatement, every operation its own numpy operation, in the header's order
    mm = ctx.matrix_apply(slot_m, u, CM1)
    r = b - f
    if with_source:
        r = r + s
    r = r - mm
    r[rows] = g - u[rows]
    assert np.array_equal(bits(r1), bits(r))
    assert np.array_equal(bits(r2), bits(r1)) and nr1 == nr2
    ref = np.linalg.norm(r)
    print("%s %s: |r| %.17g device %.17g, rel %.2e (bound %.2e)" % (which, model, ref, nr1, abs(nr1 - ref) / ref, n * EPS))
    assert abs(nr1 - ref) <= n * EPS * ref
    assert ctx.newton_info()["residuals"] == 2
    # the held right-hand side is untouched by the residual
    ctx.newton_end()
    assert np.array_equal(bits(ctx.rhs_get()), bits(b))
    assert np.array_equal(bits(ctx.solution_get()), bits(u))


# ---------------------------------------------------------------------------------------------------------------------------
# 3  state handling
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["p1_cube4", "p1_square6"])      # 375 rows (odd: the scalar tail row) and 98
def test_begin_update_end(fedd_lib, ctx, which):
    lib = fedd_lib
    m = get_mesh(lib, which)
    dim = m["dim"]
    model = hr.STVK
    setup_masses(lib, ctx, m)
    own = own_dofs(m)
    n = own.shape[0]
    assert n % 2 == (1 if which == "p1_cube4" else 0)
    rng = np.random.default_rng(9)
    u0 = smooth_displacement(m).ravel()[own]
    b = rng.uniform(-1.0, 1.0, n)
    d = 0.01 * rng.uniform(-1.0, 1.0, n)
    ctx.solution_set(u0)
    ctx.rhs_set(b)
    ctx.newton_begin()
    assert ctx.newton_info() == {"active": True, "n": n, "have_source": False, "force_fresh": False, "residuals": 0, "updates": 0}
    ctx.rhs_set(rng.uniform(-1.0, 1.0, n))      # the system's right-hand side is free for the residual
    ctx.solution_set(d)                          # what a solve leaves
    nd = ctx.newton_update(1.0)
    assert abs(nd - np.linalg.norm(d)) <= n * EPS * np.linalg.norm(d)
    assert np.array_equal(bits(ctx.newton_get()), bits(u0 + d))
    # the nodal vector field followed: the force of u_k equals the force of the same vector given by fedd_velocity_set
    ctx.assemble_hyperelastic(model_id(lib, model), PARAMS[model], lib.HYPER_FORCE)
    f_dev = ctx.hyperelastic_force_get()
    ug = np.zeros(dim * int(m["n_global"]))
    ug[own] = u0 + d
    set_u(ctx, m, ug)
    ctx.assemble_hyperelastic(model_id(lib, model), PARAMS[model], lib.HYPER_FORCE)
    assert np.array_equal(bits(f_dev), bits(ctx.hyperelastic_force_get()))
    nd2 = ctx.newton_update(0.5)
    assert nd2 == nd
    assert np.array_equal(bits(ctx.newton_get()), bits((u0 + d) + (0.5 * d)))
    assert ctx.newton_info()["updates"] == 2
    ctx.newton_end()
    assert np.array_equal(bits(ctx.solution_get()), bits((u0 + d) + (0.5 * d)))
    assert np.array_equal(bits(ctx.rhs_get()), bits(b))
    assert not ctx.newton_info()["active"]


def test_state_errors(fedd_lib, ctx):
    lib = fedd_lib
    m = get_mesh(lib, "p1_cube4")
    setup_masses(lib, ctx, m)
    nh = (model_id(lib, hr.NEOHOOKE), PARAMS[hr.NEOHOOKE])
    for call in (lambda: ctx.newton_update(1.0), lambda: ctx.newton_end(), lambda: ctx.newton_source_set(np.zeros(375)),
                 lambda: ctx.newton_residual(SLOT_MD, CM1), lambda: ctx.newton_get()):
        with pytest.raises(lib.FeddError, match="no Newton state"):
            call()
    ctx.newton_begin()
    with pytest.raises(lib.FeddError, match="no force vector"):
        ctx.newton_residual(SLOT_MD, CM1)
    ctx.assemble_hyperelastic(*nh, lib.HYPER_FORCE)
    ctx.newton_residual(SLOT_MD, CM1)
    ctx.newton_update(1.0)
    with pytest.raises(lib.FeddError, match="stale"):
        ctx.newton_residual(SLOT_MD, CM1)
    ctx.assemble_hyperelastic_time(*nh, SLOT_MD, CM1)
    ctx.newton_residual(SLOT_MD, CM1)
    ctx.newton_begin()                           # a new step: the force of the last one is stale again
    with pytest.raises(lib.FeddError, match="stale"):
        ctx.newton_residual(SLOT_MD, CM1)
    ctx.assemble_hyperelastic(*nh, lib.HYPER_FORCE)
    with pytest.raises(lib.FeddError, match="slot %d is empty" % SLOT_EMPTY):
        ctx.newton_residual(SLOT_EMPTY, CM1)
    with pytest.raises(lib.FeddError, match="out of range"):
        ctx.newton_residual(9, CM1)
    ctx.pattern_build(1, lib.BLOCK_SCALAR)
    ctx.assemble(lib.FORM_MASS)
    ctx.matrix_store(4)
    ctx.pattern_build(3, lib.BLOCK_FULL)
    ctx.newton_begin()
    ctx.assemble_hyperelastic(*nh, lib.HYPER_FORCE)
    with pytest.raises(lib.FeddError, match="system's size"):
        ctx.newton_residual(4, CM1)              # 125 rows against 375
    # a scalar system has no nodal vector field to share with the solution
    ctx.pattern_build(1, lib.BLOCK_SCALAR)
    with pytest.raises(lib.FeddError, match="dim dofs per node"):
        ctx.newton_begin()
    # a new mesh ends the state
    ctx.pattern_build(3, lib.BLOCK_FULL)
    ctx.newton_begin()
    ctx.mesh_set_dict(m)
    ctx.pattern_build(3, lib.BLOCK_FULL)
    with pytest.raises(lib.FeddError, match="no Newton state"):
        ctx.newton_update(1.0)


def test_more_than_one_rank_is_an_error_that_says_so(fedd_lib):
    c = fedd_lib.Context(device=0, rank=0, nranks=2, nccl_id=None)
    try:
        z = np.zeros(8)
        p = fedd_lib._p(z, fedd_lib._f64p)
        L = c._L
        for name, call in (("fedd_newton_begin", lambda: L.fedd_newton_begin(c._h)),
                           ("fedd_newton_source_set", lambda: L.fedd_newton_source_set(c._h, p)),
                           ("fedd_newton_residual", lambda: L.fedd_newton_residual(c._h, 0, 1.0, 0, None, None, None, None)),
                           ("fedd_newton_update", lambda: L.fedd_newton_update(c._h, 1.0, None)),
                           ("fedd_newton_end", lambda: L.fedd_newton_end(c._h)),
                           ("fedd_newton_get", lambda: L.fedd_newton_get(c._h, p))):
            assert call() != 0, name
            assert "%s: one rank only (a context with 2 ranks was given)" % name in L.fedd_last_error().decode(), name
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 4  one Newmark-Newton step: device-resident against host vectors
# ---------------------------------------------------------------------------------------------------------------------------
DT4 = 0.25
CM4 = 1.0 / ((DT4 * DT4) * BETA)
GM = dict(rtol=1e-13, max_it=600, restart=200, use_prec=True)
NEWTON_TOL, NEWTON_MAX = 1e-12, 25


def step_inputs(lib, ctx, m, force):
    """u_n (smooth, zero on the Dirichlet rows) and b = M t + load, t a smooth vector: the right-hand side of a step"""
    dim = m["dim"]
    own = own_dofs(m)
    is_dir = hr.dirichlet_mask(m)[own]
    un = 0.05 * smooth_displacement(m, scale=0.02).ravel()[own]
    un[is_dir] = 0.0
    ctx.assemble_rhs([force, 0.0, 0.0] if dim == 3 else [0.0, force])
    load = ctx.rhs_get()
    t = CM4 * un + 0.3 * np.sin(np.arange(un.shape[0]))
    b = ctx.matrix_apply(SLOT_MD, t) + load
    return un, b, is_dir


def host_vector_step(lib, ctx, m, model, un, b, is_dir):
    """the step with the entries of the parent commit and host arrays"""
    mid, p = model_id(lib, model), PARAMS[model]
    own = own_dofs(m)
    dim = m["dim"]
    u = un.copy()
    ug = np.zeros(dim * int(m["n_global"]))
    ratios, r0 = [], None
    for it in range(NEWTON_MAX + 1):
        ug[own] = u
        set_u(ctx, m, ug)
        ctx.assemble_hyperelastic(mid, p)
        ctx.matrix_store(SLOT_FREE)
        ctx.matrix_combine(SLOT_MD, CM4, SLOT_FREE, 1.0)
        f = ctx.hyperelastic_force_get()
        mm = ctx.matrix_apply(SLOT_MD, u, CM4)
        r = (b - f) - mm
        r[is_dir] = 0.0 - u[is_dir]
        nr = np.linalg.norm(r)
        r0 = nr if r0 is None else r0
        ratios.append(nr / r0)
        if ratios[-1] <= NEWTON_TOL:
            return u, ratios, it
        ctx.dirichlet([2])
        ctx.schwarz_setup(1, lib.COMBINE_RESTRICTED)
        du, _, _ = ctx.gmres(r, **GM)
        u = u + du
    raise RuntimeError("host-vector Newton did not reach %g: %r" % (NEWTON_TOL, ratios))


def device_step(lib, ctx, m, model, un, b, slot_m=SLOT_MD, cm=CM4, source=None, tol=NEWTON_TOL):
    """the same step with the iterate, the residual and the update on the device; leaves u_{n+1} in the solution vector"""
    mid, p = model_id(lib, model), PARAMS[model]
    ctx.solution_set(un)
    ctx.rhs_set(b)
    ctx.newton_begin()
    if source is not None:
        ctx.newton_source_set(source)
    ratios, r0 = [], None
    for it in range(NEWTON_MAX + 1):
        ctx.assemble_hyperelastic_time(mid, p, slot_m, cm)
        ctx.dirichlet([2])
        nr = ctx.newton_residual(slot_m, cm, [2])
        r0 = nr if r0 is None else r0
        ratios.append(nr / r0)
        if ratios[-1] <= tol:
            ctx.newton_end()
            return ctx.solution_get(), ratios, it
        ctx.schwarz_setup(1, lib.COMBINE_RESTRICTED)
        ctx.gmres(None, want_x=False, **GM)
        ctx.newton_update(1.0)
    raise RuntimeError("device Newton did not reach %g: %r" % (tol, ratios))


def test_one_step_device_resident_against_host_vectors(fedd_lib, ctx):
    lib = fedd_lib
    m = get_mesh(lib, "p1_cube4")
    model = hr.NEOHOOKE
    setup_masses(lib, ctx, m)
    un, b, is_dir = step_inputs(lib, ctx, m, -0.01)
    u_h, ratios_h, its_h = host_vector_step(lib, ctx, m, model, un, b, is_dir)
    ctx.pattern_build(3, lib.BLOCK_FULL)
    u_d, ratios_d, its_d = device_step(lib, ctx, m, model, un, b)
    print("host-vector %r\ndevice      %r" % (ratios_h, ratios_d))
    assert its_d == its_h and its_d >= 2
    assert np.abs(u_d - u_h).max() <= 1e-10 * np.abs(u_h).max()
    assert np.abs(u_d - un).max() > 1e-3 * np.abs(u_h).max()        # the step moved
    info = ctx.newton_info()
    assert info["residuals"] == its_d + 1 and info["updates"] == its_d


# ---------------------------------------------------------------------------------------------------------------------------
# 5  small amplitudes: the nonlinear step tends to the linear one, at second order
# ---------------------------------------------------------------------------------------------------------------------------
MU5, NU5, RHO5, DT5 = 0.3571, 0.4, 1.0, 0.5
LAM5 = hr.stvk_params(MU5, NU5)[0]
CM5 = 1.0 / ((DT5 * DT5) * BETA)
AMP = 0.02
N_STEPS = 2


def newmark_coefs(dt, beta, gamma):
    return dict(cuu=1.0 / ((dt * dt) * beta), cuv=1.0 / (dt * beta), cuw=(0.5 - beta) / beta,
                cvu=gamma / (dt * beta), cvv=1.0 - (gamma / beta), cvw=(dt * (beta - (0.5 * gamma))) / beta)


def newmark_advance(k, u, un, v, w, first):
    """the header's formulas of fedd_newmark_advance"""
    if not first:
        d = u - un
        v, w = ((k["cvu"] * d) + (k["cvv"] * v)) + (k["cvw"] * w), ((k["cuu"] * d) - (k["cuv"] * v)) - (k["cuw"] * w)
    return u.copy(), v, w, ((k["cuu"] * u) + (k["cuv"] * v)) + (k["cuw"] * w)


_rest5 = {}


def restatement_two_steps(lib, amp):
    """(u_nl, u_lin) after N_STEPS steps in global ids: hyperelastic_ref tangent and force, oracle mass and linear elasticity,
    sparse direct solves, Newton to 1e-12 of the step's first residual"""
    if amp in _rest5:
        return _rest5[amp]
    from test_gpu_parity import oracle_mesh
    m = get_mesh(lib, "p1_square6")
    om = oracle_mesh(m)
    dim = 2
    n = dim * int(m["n_global"])
    M = (RHO5 * fo.assembly_mass(om, "Vector")).tocsr()
    Kl = fo.assembly_linelas(om, LAM5, MU5).tocsr()
    fr = fo.assembly_rhs(om, [0.0, 1.0], "Vector", 0)
    gd = (dim * om.gid_rep[:, None] + np.arange(dim)[None, :]).ravel()
    f_unit = fo.export_add(fr, gd, n)
    is_dir = hr.dirichlet_mask(m)
    k = newmark_coefs(DT5, BETA, GAMMA)
    out = []
    for nonlinear in (True, False):
        u, un, v, w = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
        first = True
        for step in range(N_STEPS):
            un, v, w, t = newmark_advance(k, u, un, v, w, first)
            first = False
            b = M @ t + amp * f_unit
            if not nonlinear:
                A, rhs = fo.set_dirichlet((k["cuu"] * M + Kl).tocsr(), b.copy(), is_dir, 0.0)
                u = fo.direct_solve(A, rhs)
                continue
            r0 = None
            for it in range(30):
                K, f, _ = hr.assemble(m, u.reshape(-1, dim)[m["gid_rep"]], hr.STVK, (LAM5, MU5))
                r = (b - f) - k["cuu"] * (M @ u)
                r[is_dir] = 0.0 - u[is_dir]
                nr = np.linalg.norm(r)
                r0 = nr if r0 is None else r0
                if os.environ.get("FEDD_TEST_VERBOSE"):
                    print("  restatement a = %g step %d it %d: |r| / |r_0| %.3e" % (amp, step, it, nr / r0))
                if nr <= 1e-12 * r0:
                    break
                A, rhs = fo.set_dirichlet((k["cuu"] * M + K).tocsr(), r, is_dir, 0.0)
                rhs[is_dir] = r[is_dir]
                u = u + fo.direct_solve(A, rhs)
            else:
                raise RuntimeError("the restatement's Newton loop did not converge")
        out.append(u)
    _rest5[amp] = tuple(out)
    return _rest5[amp]


def device_two_steps(lib, ctx, m, amp, nonlinear):
    own = own_dofs(m)
    ctx.pattern_build(2, lib.BLOCK_FULL)
    ctx.assemble_rhs([0.0, 1.0])
    f_unit = ctx.rhs_get()
    ctx.solution_set(np.zeros(own.shape[0]))
    ctx.newmark_begin()
    for step in range(N_STEPS):
        ctx.newmark_advance(SLOT_MD, DT5, BETA, GAMMA, 1.0)
        ctx.rhs_axpy(amp, f_unit)
        if nonlinear:
            b = ctx.rhs_get()
            device_step(lib, ctx, m, hr.STVK, ctx.solution_get(), b, cm=CM5, tol=1e-12)
        else:
            ctx.matrix_combine(SLOT_MD, CM5, SLOT_A, 1.0)
            ctx.dirichlet([2])
            ctx.schwarz_setup(1, lib.COMBINE_RESTRICTED)
            ctx.gmres(None, want_x=False, **GM)
    return ctx.solution_get()


def test_small_amplitude_limit_is_the_linear_newmark_path(fedd_lib, ctx):
    """Saint Venant-Kirchhoff on the 6 x 6 square, body force (0, a), density 1, dt = 0.5, beta = 1/4, gamma = 1/2, two steps,
    against FEDD_FORM_LINELAS + fedd_newmark_* with the same lambda, mu.  d(a) = max |u_nl - u_lin| is second order in a: the
    ratio d(a / 2) / d(a) is 1/4 to leading order and must stay below 0.35.

    a = 0.02, chosen on the CPU with the restatement above (hyperelastic_ref + scipy direct solves), which gave
    max|u| = 6.34e-3, d(a) = 2.351e-5 = 3.7e-3 max|u| (ten orders above the 1e-13 solve floor), d(a / 2) = 5.895e-6, ratio 0.2507;
    the test asserts those conditions on the restatement again before it looks at the device."""
    lib = fedd_lib
    m = get_mesh(lib, "p1_square6")
    own = own_dofs(m)
    d_rest, umax = {}, {}
    for amp in (AMP, 0.5 * AMP):
        u_nl, u_lin = restatement_two_steps(lib, amp)
        d_rest[amp] = np.abs(u_nl - u_lin).max()
        umax[amp] = np.abs(u_lin).max()
    ratio_rest = d_rest[0.5 * AMP] / d_rest[AMP]
    print("restatement: max|u| %.3e, d(a) %.3e, d(a/2) %.3e, ratio %.4f" % (umax[AMP], d_rest[AMP], d_rest[0.5 * AMP], ratio_rest))
    assert d_rest[0.5 * AMP] >= 1e3 * 1e-13 * umax[AMP]
    assert ratio_rest < 0.35
    setup_masses(lib, ctx, m, density=RHO5)
    ctx.pattern_build(2, lib.BLOCK_FULL)
    ctx.assemble(lib.FORM_LINELAS, [LAM5, MU5])
    ctx.matrix_store(SLOT_A)
    d_dev = {}
    for amp in (AMP, 0.5 * AMP):
        u_nl = device_two_steps(lib, ctx, m, amp, True)
        u_lin = device_two_steps(lib, ctx, m, amp, False)
        d_dev[amp] = np.abs(u_nl - u_lin).max()
        ref_nl, ref_lin = restatement_two_steps(lib, amp)
        print("a = %g: device d %.3e; against the restatement: nonlinear %.2e, linear %.2e of max|u|" % (
            amp, d_dev[amp], np.abs(u_nl - ref_nl[own]).max() / umax[amp], np.abs(u_lin - ref_lin[own]).max() / umax[amp]))
        assert np.abs(u_nl - ref_nl[own]).max() <= 1e-10 * umax[amp]
    ratio = d_dev[0.5 * AMP] / d_dev[AMP]
    print("device: d(a) %.3e, d(a/2) %.3e, ratio %.4f" % (d_dev[AMP], d_dev[0.5 * AMP], ratio))
    assert ratio < 0.35

"""Diagonal / Triangular block preconditioners of the merged Stokes system (include/fedd_hip.h "Block preconditioners",
feddlib_amd/csrc/blockprec.hip; PrecBlock2x2_def.hpp:114-164): fedd_matrix_import, the apply against its host composition bit
for bit, the coupling term against scipy, solves against a direct solve, and the lifecycle of the attach.

Shapes: the 4 x 4-cell P2 / P1 channel of test_small_stokes_solve (nonzero inflow values: Dirichlet masking matters) and the 1k
cylinder with the driver's boundary conditions."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import fedd_oracle as fo

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Stokes:
    """parent context with the merged system, velocity child (import of block (0,0) + Dirichlet rows), Schur child ((1/nu) M_p)"""

    def __init__(self, lib, which, nu=1.0):
        self.lib, self.nu = lib, nu
        if which == "channel":
            self.dim = 2
            self.m1 = lib.structured_mesh(2, 1, 4)
        else:
            self.dim = 3
            self.m1 = lib.read_mesh(os.path.join(GOLD, "DFG3DCylinder_1k.mesh"), 3)
        self.mv = lib.p2_of_p1(self.m1, volume_id=0)
        self.n_p, self.nv = self.m1["xyz"].shape[0], self.mv["xyz"].shape[0]
        self.nA = self.dim * self.nv
        self.n = self.nA + self.n_p
        X, dim = self.mv["xyz"], self.dim
        if which == "channel":      # parabolic inflow on x = 0, no-slip walls, natural outflow
            inflow = X[:, 0] < 1e-12
            wall = (X[:, 1] < 1e-12) | (X[:, 1] > 1 - 1e-12)
            self.bc_nodes = np.nonzero(inflow | wall)[0]
            self.bc_vals = np.zeros((self.bc_nodes.shape[0], dim))
            free_in = inflow[self.bc_nodes] & ~wall[self.bc_nodes]
            y = X[self.bc_nodes, 1]
            self.bc_vals[free_in, 0] = (4.0 * y * (1.0 - y))[free_in]
        else:                       # no-slip on flags 1 and 4, parabolic inflow on flag 2, flag 3 natural (stokes/main.cpp:80-88, 267-296)
            flag, H = self.mv["flag_uni"], 0.41
            self.bc_nodes = np.nonzero(np.isin(flag, (1, 2, 4)))[0]
            self.bc_vals = np.zeros((self.bc_nodes.shape[0], dim))
            infl = flag[self.bc_nodes] == 2
            y, z = X[self.bc_nodes, 1], X[self.bc_nodes, 2]
            self.bc_vals[infl, 0] = (16.0 * y * (H - y) * z * (H - z) / H ** 4)[infl]
        self.bc_rows = (dim * self.bc_nodes[:, None] + np.arange(dim)[None, :]).ravel()
        self.is_dir = np.zeros(self.nA, dtype=bool)
        self.is_dir[self.bc_rows] = True
        self.p = lib.Context(device=0)
        self.v = lib.Context(device=0)
        self.s = lib.Context(device=0)
        p = self.p
        p.mesh_set_dict(self.mv)
        p.pattern_build(dim, lib.BLOCK_DIAG)
        p.assemble(lib.FORM_LAPLACE_VEC)
        p.matrix_scale(-1, nu)
        p.matrix_store(0)
        p.assemble_div(self.n_p, 1, 2)
        p.matrix_scale(1, -1.0)
        p.matrix_scale(2, -1.0)
        self.slot_f = 0
        self.merge()
        self.v.mesh_set_dict(self.mv)
        self.import_velocity()
        self.s.mesh_set_dict(self.m1)
        self.s.pattern_build(1, lib.BLOCK_SCALAR)
        self.s.assemble(lib.FORM_MASS)
        self.s.matrix_scale(-1, 1.0 / nu)

    def merge(self):
        self.p.block_merge(self.slot_f, 2, 1, -1)
        self.p.rhs_set(np.zeros(self.n))
        self.p.dirichlet_rows(self.bc_rows, self.bc_vals.ravel())

    def import_velocity(self):
        self.v.matrix_import(self.p, self.slot_f)
        self.v.dirichlet_nodes(self.bc_nodes, self.bc_vals)

    def setup_velocity(self, two_level=False):
        """The P2 velocity rows of the 3D mesh couple a node to so many others that a box plus one graph layer exceeds the 256 dofs
        of the dense local solver: there the boxes go without overlap (9 nodes, 27 dofs).  The 2D channel takes the default
        boxes with overlap 1.  One-level and two-level children differ by the coarse level alone."""
        lib, v = self.lib, self.v
        overlap = 1 if self.dim == 2 else 0
        if two_level:
            v.schwarz_set_coarse(8)
            v.schwarz_setup(overlap, lib.COMBINE_RESTRICTED, two_level=1, coarse_kind=lib.COARSE_Q1)
        else:
            v.schwarz_setup(overlap, lib.COMBINE_RESTRICTED)

    def setup_children(self, two_level=False):
        lib = self.lib
        self.setup_velocity(two_level)
        if two_level:
            self.s.schwarz_set_coarse(8)
            self.s.schwarz_setup(1, lib.COMBINE_RESTRICTED, two_level=1, coarse_kind=lib.COARSE_Q1)
        else:
            self.s.schwarz_setup(1, lib.COMBINE_RESTRICTED)

    def host_apply(self, kind, scale, r):
        """the composition the header states, out of the public pieces"""
        r_u, r_p = r[:self.nA], r[self.nA:]
        z_p = scale * self.s.schwarz_apply(r_p)
        if kind == self.lib.BLOCKPREC_DIAGONAL:
            return np.concatenate([self.v.schwarz_apply(r_u), z_p]), None
        bt = self.p.matrix_apply(2, z_p, 1.0)
        t = r_u - bt
        t[self.is_dir] = r_u[self.is_dir]
        return np.concatenate([self.v.schwarz_apply(t), z_p]), bt

    def close(self):
        for c in (self.p, self.v, self.s):
            c.close()


@pytest.fixture(scope="module")
def channel(fedd_lib):
    st = Stokes(fedd_lib, "channel")
    yield st
    st.close()


@pytest.fixture(scope="module")
def channel_nu(fedd_lib):
    """the channel at nu = 1e-3 (the viscosity of cfg 4): A = nu K and the Schur child's (1 / nu) M_p are both far from 1"""
    st = Stokes(fedd_lib, "channel", nu=1.0e-3)
    yield st
    st.close()


@pytest.fixture(scope="module")
def cylinder(fedd_lib):
    st = Stokes(fedd_lib, "cylinder")
    yield st
    st.close()


@pytest.fixture(scope="module")
def cylinder_direct(cylinder):
    """the merged system of the cylinder and its direct solution, computed once"""
    rowptr, col, val, _ = cylinder.p.csr_get()
    M = sp.csr_matrix((val, col, rowptr), shape=(cylinder.n, cylinder.n))
    b = cylinder.p.rhs_get()
    return M, b, fo.direct_solve(M, b)


def _csr(c):
    rowptr, col, val, _ = c.csr_get()
    n = rowptr.shape[0] - 1
    return sp.csr_matrix((val, col, rowptr), shape=(n, n))


# ---- import ------------------------------------------------------------------------------------------------------------------
def test_import_copies_the_block_exactly_and_keeps_the_structure(fedd_lib, cylinder):
    st = cylinder
    p, v = st.p, st.v
    v.matrix_import(p, 0)
    A = p.matrix_get(0)
    rowptr, col, val, gid = v.csr_get()
    assert np.array_equal(rowptr, A.indptr) and np.array_equal(col, A.indices) and np.array_equal(val, A.data)
    assert np.array_equal(gid, np.arange(st.nA)) and v.dofs == st.dim
    assert not v.rhs_get().any() and not v.solution_get().any()
    v.dirichlet_nodes(st.bc_nodes, st.bc_vals)
    st.setup_velocity()
    n0 = v.schwarz_reuse_info()["n_reused"]
    # same pattern id, other values (matrix_scale does not rewrite the pattern): values move, the structure stage is kept
    p.matrix_scale(0, 2.0)
    v.matrix_import(p, 0)
    assert np.array_equal(v.csr_get()[2], 2.0 * A.data)
    with pytest.raises(fedd_lib.FeddError, match="preconditioner requested but fedd_schwarz_setup was not called"):
        v.gmres(None, rtol=1e-8, max_it=5, restart=5, use_prec=True)          # the import dropped the setup
    v.dirichlet_nodes(st.bc_nodes, st.bc_vals)
    st.setup_velocity()
    assert v.schwarz_reuse_info() == {"last_reused": True, "n_reused": n0 + 1}
    p.matrix_scale(0, 0.5)
    assert np.array_equal(p.matrix_get(0).data, A.data)                          # (exact: powers of two)
    # errors that name the cause
    with pytest.raises(fedd_lib.FeddError, match="slot 5 of the source is empty"):
        v.matrix_import(p, 5)
    with pytest.raises(fedd_lib.FeddError, match="non-square block"):
        v.matrix_import(p, 1)
    with pytest.raises(fedd_lib.FeddError, match="size mismatch: the block has %d rows, the destination's mesh %d owned nodes" % (st.nA, st.n_p)):
        st.s.matrix_import(p, 0)
    fresh = fedd_lib.Context(device=0)
    try:
        with pytest.raises(fedd_lib.FeddError, match="carries no mesh"):
            fresh.matrix_import(p, 0)
    finally:
        fresh.close()
    st.import_velocity()        # leave the child as the other tests expect it


# ---- apply, bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["channel", "channel_nu", "cylinder"])
def test_apply_equals_the_host_composition_bit_for_bit(fedd_lib, request, which):
    st = request.getfixturevalue(which)
    st.import_velocity()
    st.setup_children()
    BT = st.p.matrix_get(2)
    assert abs(BT[st.bc_rows]).sum() > 0            # the stored B^T has NOT had its Dirichlet rows zeroed
    r = np.random.default_rng(31).standard_normal(st.n)
    for kind in (fedd_lib.BLOCKPREC_DIAGONAL, fedd_lib.BLOCKPREC_TRIANGULAR):
        for scale in (-1.0, 1.0):
            st.p.block_prec_attach(kind, st.v, st.s, scale, 2)
            z = st.p.schwarz_apply(r)
            z2 = st.p.schwarz_apply(r)
            zh, bt = st.host_apply(kind, scale, r)
            assert np.array_equal(z, zh), (which, kind, scale, np.abs(z - zh).max())
            assert np.array_equal(z, z2)
            info = st.p.block_prec_info()
            assert (info["kind"], info["schur_scale"], info["applies"]) == (kind, scale, 2)
            assert info["slot_bt"] == (2 if kind == fedd_lib.BLOCKPREC_TRIANGULAR else -1)
            if kind == fedd_lib.BLOCKPREC_TRIANGULAR:
                # t = r_u on Dirichlet rows: B^T z_p is not zero there, and leaving the mask out changes z_u
                assert np.abs(bt[st.is_dir]).max() > 0
                z_unmasked = st.v.schwarz_apply(r[:st.nA] - bt)
                assert not np.array_equal(z_unmasked, z[:st.nA])
            st.p.block_prec_detach()


def test_apply_with_a_nonsymmetric_velocity_block(fedd_lib, cylinder):
    """F = A + N(u) + W(u) in slot 4 (fedd_assemble_advection, Newton form) in the place of A"""
    st = cylinder
    X = st.mv["xyz"]
    u = np.stack([np.sin(3.0 * X[:, 1]) + 0.5, 0.3 * np.cos(2.0 * X[:, 0]), 0.2 * X[:, 0] * X[:, 2]], axis=1)
    try:
        st.p.velocity_set(u)
        st.p.assemble_advection(fedd_lib.ADV_NEWTON, 1.0, slot_add=0, slot_out=4)
        st.slot_f = 4
        st.merge()
        st.import_velocity()
        F = _csr(st.v)
        assert abs(F - F.T).max() > 1e-3 * abs(F).max()
        st.setup_children()
        r = np.random.default_rng(32).standard_normal(st.n)
        for kind in (fedd_lib.BLOCKPREC_DIAGONAL, fedd_lib.BLOCKPREC_TRIANGULAR):
            st.p.block_prec_attach(kind, st.v, st.s, -1.0, 2)
            z = st.p.schwarz_apply(r)
            zh, _ = st.host_apply(kind, -1.0, r)
            assert np.array_equal(z, zh), (kind, np.abs(z - zh).max())
            st.p.block_prec_detach()
        # the Newton loop's case: new values in slot 4, same pattern -> values-only import, structure kept
        st.p.velocity_set(0.5 * u)
        st.p.assemble_advection(fedd_lib.ADV_NEWTON, 1.0, slot_add=0, slot_out=4)
        n0 = st.v.schwarz_reuse_info()["n_reused"]
        st.import_velocity()
        assert np.array_equal(st.v.csr_get()[0], st.p.matrix_get(4).indptr)
        st.setup_velocity()
        assert st.v.schwarz_reuse_info() == {"last_reused": True, "n_reused": n0 + 1}
    finally:
        st.p.block_prec_detach()
        st.slot_f = 0
        st.merge()
        st.import_velocity()


# ---- apply, two-level children ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["channel", "cylinder"])
def test_apply_with_two_level_children(fedd_lib, request, which):
    st = request.getfixturevalue(which)
    st.import_velocity()
    st.setup_children(two_level=True)
    assert st.v.schwarz_coarse_sizes()[1] > 0 and st.s.schwarz_coarse_sizes()[1] > 0
    r = np.random.default_rng(33).standard_normal(st.n)
    for kind in (fedd_lib.BLOCKPREC_DIAGONAL, fedd_lib.BLOCKPREC_TRIANGULAR):
        st.p.block_prec_attach(kind, st.v, st.s, -1.0, 2)
        z = st.p.schwarz_apply(r)
        zh, _ = st.host_apply(kind, -1.0, r)
        err = np.abs(z - zh).max() / np.abs(zh).max()
        print("two-level children, %s, kind %d: max deviation from the host composition %.2e of max|z|" % (which, kind, err))
        np.testing.assert_allclose(z, zh, rtol=0, atol=1e-10 * np.abs(zh).max())
        st.p.block_prec_detach()


# ---- independent of the children -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["channel", "channel_nu", "cylinder"])
def test_coupling_term_against_scipy(fedd_lib, request, which):
    """P = [[F, B^T_bc], [0, -M_p / nu]] from the matrices the device holds.  With z the device's Triangular apply of r:
    the p rows of P z are -(M_p / nu) z_p and its u rows minus F z_u are B^T_bc z_p (block structure), and -- the part that tests
    the kernel -- t = r_u - B^T_bc z_p formed by scipy reproduces z_u through V alone, and z_p is -S(r_p)."""
    st = request.getfixturevalue(which)
    st.import_velocity()
    st.setup_children()
    F, Mp = _csr(st.v), _csr(st.s)           # Mp = (1 / nu) M_p as the Schur child holds it
    rowsum = np.asarray(Mp.sum(axis=1)).ravel().sum()      # sum of all entries of M_p = the area / volume of the domain
    if st.dim == 2:
        assert abs(rowsum * st.nu - 1.0) <= 1e-12        # the unit square: the 1 / nu scaling is in the child's matrix
    BT = st.p.matrix_get(2).tolil()
    BT[st.bc_rows, :] = 0.0
    BT_bc = BT.tocsr()
    P = sp.bmat([[F, BT_bc], [None, -Mp]], format="csr")
    r = np.random.default_rng(34).standard_normal(st.n)
    st.p.block_prec_attach(fedd_lib.BLOCKPREC_TRIANGULAR, st.v, st.s, -1.0, 2)
    try:
        z = st.p.schwarz_apply(r)
    finally:
        st.p.block_prec_detach()
    z_u, z_p = z[:st.nA], z[st.nA:]
    w = P @ z
    c = BT_bc @ z_p
    tol = 1e-10 * np.abs(w).max()
    np.testing.assert_allclose(w[st.nA:], -(Mp @ z_p), rtol=0, atol=tol)
    np.testing.assert_allclose(w[:st.nA] - F @ z_u, c, rtol=0, atol=tol)
    assert np.array_equal(z_p, -st.s.schwarz_apply(r[st.nA:]))
    zu_host = st.v.schwarz_apply(r[:st.nA] - c)
    np.testing.assert_allclose(z_u, zu_host, rtol=0, atol=1e-10 * np.abs(zu_host).max())
    assert np.abs(c).max() > 1e-3 * np.abs(r).max()         # the coupling term is not negligible in this check


# ---- solve -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_level", [False, True])
@pytest.mark.parametrize("kind", ["diagonal", "triangular"])
def test_solve_on_the_1k_cylinder(fedd_lib, cylinder, cylinder_direct, kind, two_level):
    """fedd_gmres at rtol 1e-12 within the 1500 iterations / restart 300 of the monolithic test of tests/test_gpu_stokes.py, x against
    fo.direct_solve at 1e-10 max|x| (the criterion of that file).  Iteration counts are printed, not asserted.  Measured (nu = 1):
    diagonal 791 / 268 iterations, error 3.8e-11 / 3.4e-11 (one-level / two-level children); triangular 317 / 191, 9.6e-11 / 8.6e-11.
    The error bar sits close to what a 1e-12 residual gives on this system; both figures are the ones the issue sets."""
    st = cylinder
    M, b, xd = cylinder_direct
    st.import_velocity()
    st.setup_children(two_level=two_level)
    k = {"diagonal": fedd_lib.BLOCKPREC_DIAGONAL, "triangular": fedd_lib.BLOCKPREC_TRIANGULAR}[kind]
    st.p.block_prec_attach(k, st.v, st.s, -1.0, 2)
    try:
        x, its, rel = st.p.gmres(b, rtol=1e-12, max_it=1500, restart=300, use_prec=True)
    finally:
        st.p.block_prec_detach()
    err = np.abs(x - xd).max() / np.abs(xd).max()
    print("1k cylinder, %s, %s children: %d GMRES iterations, relres %.2e, error vs direct solve %.2e"
          % (kind, "two-level" if two_level else "one-level", its, rel, err))
    assert rel <= 1e-12
    np.testing.assert_allclose(x, xd, rtol=0, atol=1e-10 * np.abs(xd).max())


# ---- lifecycle -------------------------------------------------------------------------------------------------------------------
def test_lifecycle(fedd_lib, channel):
    st = channel
    p, v, s = st.p, st.v, st.s
    st.import_velocity()
    st.setup_children()
    r = np.random.default_rng(35).standard_normal(st.n)
    p.block_prec_attach(fedd_lib.BLOCKPREC_TRIANGULAR, v, s, -1.0, 2)
    try:
        z1 = p.schwarz_apply(r)
        # a child that is set up again: the next apply uses the new setup
        v.schwarz_setup(2, fedd_lib.COMBINE_RESTRICTED)
        z2 = p.schwarz_apply(r)
        assert not np.array_equal(z1, z2)
        assert np.array_equal(z2, st.host_apply(fedd_lib.BLOCKPREC_TRIANGULAR, -1.0, r)[0])
        x, its, rel = p.gmres(None, rtol=1e-10, max_it=400, restart=200, use_prec=True)
        assert rel <= 1e-10
        # a child without a current setup is an error that names the child, at apply time
        st.import_velocity()
        with pytest.raises(fedd_lib.FeddError, match="the velocity child has no current fedd_schwarz_setup"):
            p.schwarz_apply(r)
        with pytest.raises(fedd_lib.FeddError, match="fedd_gmres: block preconditioner: the velocity child has no current fedd_schwarz_setup"):
            p.gmres(None, rtol=1e-10, max_it=10, restart=10, use_prec=True)
        v.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
        s.matrix_scale(-1, 1.0)
        with pytest.raises(fedd_lib.FeddError, match="the Schur complement child has no current fedd_schwarz_setup"):
            p.schwarz_apply(r)
        s.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
        assert np.array_equal(p.schwarz_apply(r), z1)
        # Triangular with an empty or misshapen B^T slot
        p.block_prec_attach(fedd_lib.BLOCKPREC_TRIANGULAR, v, s, -1.0, 5)
        with pytest.raises(fedd_lib.FeddError, match=r"slot 5 \(B\^T of the Triangular form\) is empty"):
            p.schwarz_apply(r)
        p.block_prec_attach(fedd_lib.BLOCKPREC_TRIANGULAR, v, s, -1.0, 1)
        with pytest.raises(fedd_lib.FeddError, match="slot 1 holds a %d x %d matrix, B\\^T of this system is %d x %d" % (st.n_p, st.nA, st.nA, st.n_p)):
            p.schwarz_apply(r)
        # fedd_cg on a merged system stays the error it is
        with pytest.raises(fedd_lib.FeddError, match="merged block system is not symmetric positive definite"):
            p.cg(None, rtol=1e-8, max_it=10, use_prec=True)
    finally:
        p.block_prec_detach()
    # detached: the parent's own preconditioner is in force again, and it has none
    assert p.block_prec_info()["kind"] == 0
    with pytest.raises(fedd_lib.FeddError, match="preconditioner requested but fedd_schwarz_setup was not called"):
        p.gmres(None, rtol=1e-10, max_it=10, restart=10, use_prec=True)
    with pytest.raises(fedd_lib.FeddError, match="no preconditioner"):
        p.schwarz_apply(r)
    # an unmerged parent
    q = fedd_lib.Context(device=0)
    try:
        q.mesh_set_dict(st.mv)
        q.pattern_build(st.dim, fedd_lib.BLOCK_DIAG)
        with pytest.raises(fedd_lib.FeddError, match="unmerged parent"):
            q.block_prec_attach(fedd_lib.BLOCKPREC_DIAGONAL, v, s, -1.0)
    finally:
        q.close()


def test_destroying_an_attached_child_detaches_the_parent(fedd_lib):
    st = Stokes(fedd_lib, "channel")
    try:
        st.setup_children()
        st.p.block_prec_attach(fedd_lib.BLOCKPREC_DIAGONAL, st.v, st.s, -1.0)
        r = np.random.default_rng(36).standard_normal(st.n)
        st.p.schwarz_apply(r)
        st.s.close()                                    # the child goes first
        assert st.p.block_prec_info()["kind"] == 0
        with pytest.raises(fedd_lib.FeddError, match="no preconditioner"):
            st.p.schwarz_apply(r)
        st.p.sync()
        # and a parent that goes first leaves its children usable
        s2 = fedd_lib.Context(device=0)
        st.s = s2
        s2.mesh_set_dict(st.m1)
        s2.pattern_build(1, fedd_lib.BLOCK_SCALAR)
        s2.assemble(fedd_lib.FORM_MASS)
        s2.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
        st.p.block_prec_attach(fedd_lib.BLOCKPREC_DIAGONAL, st.v, s2, -1.0)
        z = st.p.schwarz_apply(r)
        st.p.close()
        assert np.array_equal(st.v.schwarz_apply(r[:st.nA]), z[:st.nA])
    finally:
        st.close()

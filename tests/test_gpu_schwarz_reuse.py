"""The Schwarz setup keeps its structure stage (box lattice, bins, overlapping dof lists) from one setup to the next while mesh,
pattern and parameters stand (option "schwarz_reuse", default 1).  Nothing in the arithmetic changes, so every comparison here
is bit for bit against a FRESH context with schwarz_reuse = 0, which builds the structure in every setup."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M = 10            # cells per direction: 1331 dofs, 27-node boxes give 5^3 and 64-node boxes 3^3 subdomains


def _laplace(c, capi, form=None, scale=None, dofs=1):
    """pattern + matrix + load + Dirichlet, the way bench.py repeats them in front of every setup"""
    if dofs == 1:
        c.pattern_build(1, capi.BLOCK_SCALAR)
        c.assemble(capi.FORM_LAPLACE if form is None else form)
        c.assemble_rhs([1.0])
        c.dirichlet([1, 2, 3], [0.0, 0.0, 0.0])
    else:
        c.pattern_build(dofs, capi.BLOCK_FULL)
        c.assemble(capi.FORM_LINELAS, [1.0 * 2 * 0.3 / (1 - 2 * 0.3), 1.0])
        c.assemble_rhs([0.0, 1.0, 0.0])
        c.dirichlet([2], [0.0, 0.0, 0.0])
    if scale is not None:
        c.matrix_scale(-1, scale)


def _observe(c, r_seed=5, solve=True):
    """what a setup is judged by: its sizes, M^-1 r for a seeded r, and the preconditioned solve"""
    n = c.csr_sizes()[0]
    r = np.random.default_rng(r_seed).standard_normal(n)
    out = dict(info=c.schwarz_info(), z=c.schwarz_apply(r))
    if solve:
        x, its, rel = c.gmres(None, rtol=1e-10, max_it=300, restart=100, use_prec=True)
        out.update(x=x, its=its)
    return out


def _assert_same(got, ref):
    assert got["info"] == ref["info"]                     # field by field
    assert np.array_equal(got["z"], ref["z"])
    if "x" in ref:
        assert got["its"] == ref["its"]
        assert np.array_equal(got["x"], ref["x"])


def _fresh(capi, mesh, problem, params, setup, **obs):
    """the baseline: a fresh context that builds everything in its one setup"""
    c = capi.Context(device=0)
    try:
        c.set_option("schwarz_reuse", 0)
        c.mesh_set_dict(mesh)
        problem(c)
        params(c)
        setup(c)
        assert c.schwarz_reuse_info() == {"last_reused": False, "n_reused": 0}
        return _observe(c, **obs)
    finally:
        c.close()


@pytest.fixture(scope="module")
def cube(fedd_lib):
    return fedd_lib.structured_mesh(3, 1, M)


@pytest.mark.parametrize("target", [27, 64])
def test_second_setup_reuses_the_structure(fedd_lib, cube, target):
    capi = fedd_lib
    problem = lambda c: _laplace(c, capi)
    params = lambda c: c.schwarz_set_target(target, 1.0)
    setup = lambda c: c.schwarz_setup(1, capi.COMBINE_RESTRICTED)
    ref = _fresh(capi, cube, problem, params, setup)
    c = capi.Context(device=0)
    try:
        c.mesh_set_dict(cube)
        for k in range(2):
            problem(c)
            params(c)
            setup(c)
            assert c.schwarz_reuse_info() == {"last_reused": k == 1, "n_reused": k}
        _assert_same(_observe(c), ref)
        # the A/B switch: with the option off the same context builds again, and computes the same
        c.set_option("schwarz_reuse", 0)
        problem(c)
        setup(c)
        assert c.schwarz_reuse_info() == {"last_reused": False, "n_reused": 1}
        _assert_same(_observe(c), ref)
    finally:
        c.close()


@pytest.mark.parametrize("other", ["mass", "scaled"])
def test_same_pattern_other_values(fedd_lib, cube, other):
    capi = fedd_lib
    first = lambda c: _laplace(c, capi)
    second = (lambda c: _laplace(c, capi, form=capi.FORM_MASS)) if other == "mass" else (lambda c: _laplace(c, capi, scale=3.0))
    params = lambda c: c.schwarz_set_target(27, 1.0)
    setup = lambda c: c.schwarz_setup(1, capi.COMBINE_RESTRICTED)
    ref = _fresh(capi, cube, second, params, setup)
    c = capi.Context(device=0)
    try:
        c.mesh_set_dict(cube)
        first(c)
        params(c)
        setup(c)
        second(c)
        setup(c)
        assert c.schwarz_reuse_info() == {"last_reused": True, "n_reused": 1}
        _assert_same(_observe(c), ref)
    finally:
        c.close()


def _jittered(mesh, h):
    """the same topology with the interior nodes moved by up to 0.2 h (seeded): nodes change their boxes"""
    m = dict(mesh)
    xyz = np.array(mesh["xyz"], dtype=np.float64, copy=True)
    interior = np.asarray(mesh["flag_rep"]) == 0
    xyz[interior] += np.random.default_rng(17).uniform(-0.2 * h, 0.2 * h, size=xyz[interior].shape)
    m["xyz"] = xyz
    return m


CHANGES = ["target", "overlap", "scale", "combine", "mesh", "pattern"]     # what differs between the two setups


@pytest.mark.parametrize("what", CHANGES)
def test_a_changed_input_rebuilds_the_structure(fedd_lib, cube, what):
    capi = fedd_lib
    st0 = dict(mesh=cube, target=27, scale=1.0, overlap=1, combine=capi.COMBINE_RESTRICTED, dofs=1)
    st1 = dict(st0)
    if what == "target":
        st1["target"] = 64
    elif what == "overlap":
        st1["overlap"] = 2
    elif what == "scale":
        st1["scale"] = 1.3
    elif what == "combine":
        st1["combine"] = capi.COMBINE_AVERAGING
    elif what == "mesh":
        st1["mesh"] = _jittered(cube, 1.0 / M)
    elif what == "pattern":
        st1["dofs"] = 3
    keeps = what == "combine"      # the combine mode is read by the numeric stage alone

    def run(c, st):
        _laplace(c, capi, dofs=st["dofs"])
        c.schwarz_set_target(st["target"], st["scale"])
        c.schwarz_setup(st["overlap"], st["combine"])

    def gather(c):     # (the averaging apply adds with floating-point atomics: the gather form is the one that repeats its bits)
        c.set_option("apply_gather", 1)

    ref = _fresh(capi, st1["mesh"], lambda c: _laplace(c, capi, dofs=st1["dofs"]),
                 lambda c: (gather(c), c.schwarz_set_target(st1["target"], st1["scale"])),
                 lambda c: c.schwarz_setup(st1["overlap"], st1["combine"]))
    c = capi.Context(device=0)
    try:
        gather(c)
        c.mesh_set_dict(st0["mesh"])
        run(c, st0)
        assert c.schwarz_reuse_info() == {"last_reused": False, "n_reused": 0}
        if st1["mesh"] is not st0["mesh"]:
            c.mesh_set_dict(st1["mesh"])
        run(c, st1)
        assert c.schwarz_reuse_info() == {"last_reused": keeps, "n_reused": int(keeps)}
        _assert_same(_observe(c), ref)
    finally:
        c.close()


def test_refined_lattice_is_the_one_reused(fedd_lib):
    """125-node boxes on 12^3 cells: the first lattice (3^3 boxes of up to 5^3 nodes, 7^3 = 343 dofs with the overlap) exceeds
    the 256 dofs of the dense local solver, so the lattice is refined at least once before it is accepted"""
    capi = fedd_lib
    mesh = capi.structured_mesh(3, 1, 12)
    problem = lambda c: _laplace(c, capi)
    params = lambda c: c.schwarz_set_target(125, 1.0)
    setup = lambda c: c.schwarz_setup(1, capi.COMBINE_RESTRICTED)
    ref = _fresh(capi, mesh, problem, params, setup)
    assert ref["info"]["n_subdomains"] > 27 and ref["info"]["max_size"] <= 256
    c = capi.Context(device=0)
    try:
        c.mesh_set_dict(mesh)
        for _ in range(2):
            problem(c)
            params(c)
            setup(c)
        assert c.schwarz_reuse_info() == {"last_reused": True, "n_reused": 1}
        _assert_same(_observe(c), ref)
    finally:
        c.close()


def _stokes(c, capi, m1, mv):
    """Taylor-Hood channel flow as tests/test_gpu_stokes.py builds it: A, B, B^T merged into one saddle-point system"""
    dim = 2
    n_p, nv = m1["xyz"].shape[0], mv["xyz"].shape[0]
    c.pattern_build(dim, capi.BLOCK_DIAG)
    c.assemble(capi.FORM_LAPLACE_VEC)
    c.matrix_store(0)
    c.assemble_div(n_p, 1, 2)
    c.matrix_scale(1, -1.0)
    c.matrix_scale(2, -1.0)
    c.block_merge(0, 2, 1, -1)
    X = mv["xyz"]
    inflow = X[:, 0] < 1e-12
    wall = (X[:, 1] < 1e-12) | (X[:, 1] > 1 - 1e-12)
    rows, vals = [], []
    for node in np.nonzero(inflow | wall)[0]:
        for d in range(dim):
            rows.append(dim * node + d)
            y = X[node, 1]
            vals.append(4.0 * y * (1.0 - y) if (inflow[node] and not wall[node] and d == 0) else 0.0)
    c.rhs_set(np.zeros(dim * nv + n_p))
    c.dirichlet_rows(np.array(rows), np.array(vals))


def test_block_merge_rebuilds_the_structure(fedd_lib):
    capi = fedd_lib
    m1 = capi.structured_mesh(2, 1, 6)
    mv = capi.p2_of_p1(m1, volume_id=0)
    problem = lambda c: _stokes(c, capi, m1, mv)
    # (merged systems take the large-subdomain path by default, which keeps nothing: this is the box path on a merged system)
    params = lambda c: (c.set_option("schwarz_big", 0), c.schwarz_set_target(9, 1.0))
    setup = lambda c: c.schwarz_setup(1, capi.COMBINE_RESTRICTED)
    ref = _fresh(capi, mv, problem, params, setup, solve=False)
    c = capi.Context(device=0)
    try:
        c.mesh_set_dict(mv)
        for _ in range(2):
            problem(c)
            params(c)
            setup(c)
            assert c.schwarz_reuse_info() == {"last_reused": False, "n_reused": 0}
        _assert_same(_observe(c, solve=False), ref)
    finally:
        c.close()


def test_two_level_setup_on_a_reused_structure(fedd_lib, cube):
    capi = fedd_lib
    problem = lambda c: _laplace(c, capi)
    params = lambda c: c.schwarz_set_target(27, 1.0)
    two = lambda c: c.schwarz_setup(1, capi.COMBINE_RESTRICTED, two_level=1, coarse_kind=capi.COARSE_Q1)
    ref = _fresh(capi, cube, problem, params, two)
    c = capi.Context(device=0)
    try:
        c.mesh_set_dict(cube)
        problem(c)
        params(c)
        c.schwarz_setup(1, capi.COMBINE_RESTRICTED)
        problem(c)
        two(c)
        assert c.schwarz_reuse_info() == {"last_reused": True, "n_reused": 1}
        _assert_same(_observe(c), ref)
    finally:
        c.close()


def _rank_main(capi, group, rank, dec, cells, reuse, out, errs):
    """one rank of a two-rank run (threads on one GPU, as tests/test_gpu_multirank.py builds them)"""
    try:
        m = capi.structured_mesh(3, dec, cells, rank, ghosts=4)
        c = capi.Context(device=0, rank=rank, nranks=group.world, nccl_id=None)
        c.mesh_set_dict(m)
        c.halo_set_owners(m["gid_rep"], capi.structured_owner(3, dec, cells, m["gid_rep"]))
        c.comm_set_thread_group(group)
        if not reuse:
            c.set_option("schwarz_reuse", 0)
        seen = []

        def step():
            _laplace(c, capi)
            c.schwarz_set_target(27, 1.0)
            c.schwarz_setup(1, capi.COMBINE_RESTRICTED)
            seen.append(c.schwarz_reuse_info())

        step()
        res = [_observe(c, r_seed=5 + rank)]
        if reuse:
            step()                                  # both ranks keep their structure
            res.append(_observe(c, r_seed=5 + rank))
            if rank == 1:
                c.set_option("schwarz_reuse", 0)    # one rank cannot keep its own: both build again
            step()
            res.append(_observe(c, r_seed=5 + rank))
        out[rank] = dict(seen=seen, res=res)
        c.close()
    except Exception as e:      # pragma: no cover
        import traceback
        errs.append("rank %d: %s\n%s" % (rank, e, traceback.format_exc()))
        try:
            group._barrier.abort()
        except Exception:
            pass


def _two_ranks(capi, reuse):
    dec, cells = (1, 1, 2), [6, 6, 6]
    group = capi.ThreadGroup(2, timeout=30.0)       # a rank left alone in a collective gives up instead of waiting
    out, errs = [None] * 2, []
    th = [threading.Thread(target=_rank_main, args=(capi, group, r, dec, cells, reuse, out, errs), daemon=True) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=90)
    assert not errs, "\n".join(errs)
    assert all(o is not None for o in out), "a rank did not finish"
    return out


def test_two_ranks_take_the_same_decision(fedd_lib):
    capi = fedd_lib
    ref = _two_ranks(capi, reuse=False)
    got = _two_ranks(capi, reuse=True)
    for rank in range(2):
        assert ref[rank]["seen"] == [{"last_reused": False, "n_reused": 0}]
        assert got[rank]["seen"] == [{"last_reused": False, "n_reused": 0}, {"last_reused": True, "n_reused": 1},
                                     {"last_reused": False, "n_reused": 1}]
        for res in got[rank]["res"]:
            _assert_same(res, ref[rank]["res"][0])

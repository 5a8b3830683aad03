"""The launch shapes that only workload-sized runs reach, forced at sizes that run in seconds.

Several hot kernels pick their launch shape from the problem size (batches per workgroup of the Schwarz apply, column groups per
workgroup of the Gram-Schmidt dot sweeps, columns per flight of the stacked apply, rows per workgroup of the assembly), and the
small meshes of the suite always get the small-problem shape: loops that never make a second trip, prefetches that never leave
their clamp, tails that are never partial.  Every shape has an option that forces it; here each forced shape is held against the
float64 numpy / scipy reference of the operation (fo.RAS, fo.CoarseGDSW, fo.direct_solve, the oracle's assembly, an
extended-precision row sum) AND against the default shape -- bit for bit where the products and their summation order do not
depend on the shape, which is the case everywhere but in the iterative solves.

Tolerances are the project's: 1e-10 max |reference| for operator applications and K0^-1, 1e-11 between two device paths, RTOL
for matrices and solves."""
import numpy as np
import pytest

import fedd_oracle as fo
from test_gpu_dedupe import CASES as DEDUPE_CASES, problem as dedupe_problem
from test_gpu_distorted import _spmv_exact_check, check_mesh, distorted
from test_gpu_nonsymmetric import box_lists, device_system, read_back
from test_gpu_parity import RTOL, _setup_laplace, assert_matrix_close, csr_global, oracle_mesh
from test_nonsymmetric_inputs import lattice_bins

pytestmark = pytest.mark.gpu

AM_MB = 16          # places (subdomains) per batch of the matrix-core apply kernels


# ---- 1. Schwarz apply under forced spans -------------------------------------------------------------------------------------
# the two 3D Laplace entries of test_gpu_dedupe.CASES on the 14^3-cell cube, and the constant-velocity nonsymmetric system on it
SPAN_SYSTEMS = [("laplace",) + t[2:4] for t in DEDUPE_CASES if t[:3] == ("laplace", 3, 14)] + [("constant", 14, 8)]
assert len(SPAN_SYSTEMS) == 3
BT_SPANS = (16, 32, 48, 80, 112, 336)           # batches per workgroup 1, 2, 3, 5, 7, 21 (pairwise coprime beyond 1)
MFMA_SPANS = (16, 32, 40, 64, 96, 128)          # places per workgroup; 40 is rounded up to 48 (whole 16-place batches)
_SPAN_REF = {}


def host_batch_table(A, lists):
    """The batch table of k_apply_bt restated on the host: boxes whose local matrices agree (dof lists equal up to a shift, rows
    with the same values at the same column offsets, to nine digits of the matrix scale) share an inverse, the box of lowest
    index is their representative; the apply order is the stable sort of the boxes by representative; a run of equal
    representatives is cut into batches of sixteen.  Returns (representative of every batch in table order, distinct matrices)."""
    row = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    fp = np.zeros(A.shape[0])
    np.add.at(fp, row, A.data * np.cos(1.0 + 0.37 * (A.indices - row)))
    fp = np.round(fp / np.abs(A.data).max(), 9)
    first, rep = {}, []
    for b, (own, ext) in enumerate(lists):
        idx = np.concatenate([own, ext])
        rep.append(first.setdefault((own.shape[0], (idx - idx[0]).tobytes(), fp[idx].tobytes()), b))
    rep = np.asarray(rep)
    batch_rep = []
    for r_ in np.unique(rep):                     # (increasing representative = the sorted order; members stay in box order)
        batch_rep += [int(r_)] * (-(-int(np.count_nonzero(rep == r_)) // AM_MB))
    return np.asarray(batch_rep), len(first)


def _span_reference(L, c, which, M, target):
    """assembles the system on c; returns (matrix read back, dofs per node, boxes, largest, r, fo.RAS's z, batch table)"""
    if which == "laplace":
        m, _, dofs = dedupe_problem(L, c, "laplace", 3, M)
        A = read_back(c)
    else:
        m, A, _ = device_system(L, c, 3, M, "constant")
        dofs = 3
    key = (which, M, target)
    if key not in _SPAN_REF:
        node_bin, nb, largest = lattice_bins(A, m["xyz"], target, dofs, 1)
        r = np.random.default_rng(M + target).standard_normal(A.shape[0])
        zo = fo.RAS(A, node_bin, nb, dofs=dofs, overlap=1).apply(r)
        batch_rep, n_distinct = host_batch_table(A, box_lists(A, node_bin, nb, dofs, 1))
        _SPAN_REF[key] = (nb, largest, r, zo, batch_rep, n_distinct)
    return (dofs,) + _SPAN_REF[key]


def _apply_fresh(c, r, span=0):
    """schwarz_apply(r) under apply_span `span`, after an apply of another vector under the default span: the device keeps z
    between two calls, so a row that the kernel fails to write under a forced span would otherwise still hold the right value
    from the apply before (the mutation that shortens a workgroup's range by one batch passed that way)"""
    c.set_option("apply_span", 0)
    c.schwarz_apply(1.0 - 3.0 * r[::-1])
    c.set_option("apply_span", span)
    return c.schwarz_apply(r)


def _shared_setup(L, c, target, kind, nb, largest):
    c.schwarz_set_target(target, 1.0)
    c.set_option("schwarz_dedupe", 1)
    c.set_option("apply_kind", kind)
    c.set_option("apply_span", 0)
    c.schwarz_setup(1, L.COMBINE_RESTRICTED)
    info = c.schwarz_info()
    assert info["n_subdomains"] == nb and info["max_size"] == largest
    # the matrix-core family is taken (most boxes share an inverse), and on the batch table (every box conforms)
    assert info["n_unique"] * 4 <= nb and info["n_conforming"] == nb, info
    return info


@pytest.mark.parametrize("which,M,target", SPAN_SYSTEMS, ids=["%s-%d-%d" % s for s in SPAN_SYSTEMS])
def test_batch_table_apply_under_forced_spans(fedd_lib, which, M, target):
    """k_apply_bt (apply_kind 4, restricted combination, every box conforming) with apply_span 16, 32, 48, 80, 112, 336 and 16 x
    (batches + 1): bspan = ceil(span / 16) = 1, 2, 3, 5, 7, 21 batches per workgroup and one workgroup that walks the whole
    table; the default rule, ceil(batches / (256 occ)), gives 1 on all three systems.  From two batches on the loop makes further
    trips: the descriptor prefetch two ahead (clamped to b_end - 1), the reload of the dof offsets where the representative
    changes inside a range, and b_end = min(nbatch, b + bspan) of a partial last range.
    Instantiations (row tiles RT, column steps KW) by the largest box: Laplace 27-node boxes 27 + 74 = 101 dofs: <2, 10>, 125
    boxes; Laplace 8-node boxes 8 + 38 = 46: <2, 10>, 729 boxes; constant-velocity system (3 dofs per node, lattice refined to
    8-node boxes) 24 + 114 = 138: <2, 10>, 729 boxes.  The batch count is restated on the host (host_batch_table) and held
    against fedd_schwarz_unique; asserted: some span leaves a last range shorter than bspan, and some range of more than one and
    fewer than all batches holds two representatives.
    z against fo.RAS on the matrix read back (1e-10 max |z|), and bit for bit the z of the default span: a box's product does not
    depend on the workgroup that takes it.
    Measured: 1.2e-15, 1.3e-15 and 1.6e-15 of max |z| against the oracle (the same at every span), every span bit for bit
    the default; 28, 80 and 80 batches of 27, 64 and 64 distinct matrices; a partial last range at bspan 3, 5, 21 (28 batches)
    and 3, 7, 21 (80), two representatives in a range at every bspan from 2 on."""
    L = fedd_lib
    c = L.Context(device=0)
    try:
        dofs, nb, largest, r, zo, batch_rep, n_distinct = _span_reference(L, c, which, M, target)
        info = _shared_setup(L, c, target, 4, nb, largest)
        assert info["n_unique"] == n_distinct, (info, n_distinct)
        nbatch = batch_rep.shape[0]
        scale = np.abs(zo).max()
        z_def = _apply_fresh(c, r)
        np.testing.assert_allclose(z_def, zo, rtol=0, atol=1e-10 * scale)
        partial, mixed, worst = [], [], 0.0
        for span in BT_SPANS + (AM_MB * (nbatch + 1),):
            bspan = -(-span // AM_MB)
            nwg = -(-nbatch // bspan)
            if nbatch - (nwg - 1) * bspan < bspan:
                partial.append(bspan)
            if 1 < bspan < nbatch and any(np.unique(batch_rep[w * bspan:(w + 1) * bspan]).shape[0] > 1 for w in range(nwg)):
                mixed.append(bspan)
            z = _apply_fresh(c, r, span)
            err = float(np.abs(z - zo).max() / scale)
            worst = max(worst, err)
            print("%s M %d target %d: %d boxes, %d batches, %d distinct; span %d = %d batches x %d workgroups: error %.2e, "
                  "bits equal %s" % (which, M, target, nb, nbatch, n_distinct, span, bspan, nwg, err, np.array_equal(z, z_def)))
            np.testing.assert_allclose(z, zo, rtol=0, atol=1e-10 * scale, err_msg="apply_span %d" % span)
            assert np.array_equal(z, z_def), "apply_span %d: %d entries differ from the default span" \
                % (span, np.count_nonzero(z != z_def))
        print("worst %.2e; partial last range at bspan %s; two representatives in a range at bspan %s" % (worst, partial, mixed))
        assert partial and partial[0] < nbatch, (nbatch, partial)
        assert mixed, (nbatch, batch_rep)
    finally:
        c.set_option("apply_span", 0)
        c.set_option("apply_kind", 0)
        c.set_option("schwarz_dedupe", 1)
        c.close()


@pytest.mark.parametrize("which,M,target", SPAN_SYSTEMS, ids=["%s-%d-%d" % s for s in SPAN_SYSTEMS])
def test_chunk_record_apply_under_forced_spans(fedd_lib, which, M, target):
    """k_apply_mfma (apply_kind 6: chunk records instead of the batch table) with apply_span 16, 32, 40, 64, 96, 128 places per
    workgroup; the rule gives 32 below 48k subdomains, 64 / 96 / 128 above, and 40 is rounded up to 48 (whole 16-place batches).
    From 96 on a workgroup crosses into a second 64-place chunk (the records requested a chunk ahead), 16 ... 48 end inside the
    first.  125 and 729 boxes: no multiple of 128 (nor of any span), so the last workgroup's range is cut by p_end =
    min(nsub, (wg + 1) span).  Same systems and instantiations <2, 10> as test_batch_table_apply_under_forced_spans.
    z against fo.RAS on the matrix read back (1e-10 max |z|); bit for bit the z of the default span, and of the batch-table kernel
    (the same products in the same order).
    Measured: 1.2e-15, 1.3e-15 and 1.6e-15 of max |z| against the oracle, every span bit for bit the default."""
    L = fedd_lib
    c = L.Context(device=0)
    try:
        dofs, nb, largest, r, zo, batch_rep, n_distinct = _span_reference(L, c, which, M, target)
        _shared_setup(L, c, target, 4, nb, largest)
        assert nb % 128 != 0
        z_bt = _apply_fresh(c, r)
        c.set_option("apply_kind", 6)
        z_def = _apply_fresh(c, r)
        scale = np.abs(zo).max()
        np.testing.assert_allclose(z_def, zo, rtol=0, atol=1e-10 * scale)
        assert np.array_equal(z_def, z_bt)
        worst = 0.0
        for span in MFMA_SPANS:
            z = _apply_fresh(c, r, span)
            err = float(np.abs(z - zo).max() / scale)
            worst = max(worst, err)
            print("%s M %d target %d: %d boxes; span %d: error %.2e, bits equal %s"
                  % (which, M, target, nb, span, err, np.array_equal(z, z_def)))
            np.testing.assert_allclose(z, zo, rtol=0, atol=1e-10 * scale, err_msg="apply_span %d" % span)
            assert np.array_equal(z, z_def), "apply_span %d: %d entries differ from the default span" \
                % (span, np.count_nonzero(z != z_def))
        print("worst %.2e" % worst)
    finally:
        c.set_option("apply_span", 0)
        c.set_option("apply_kind", 0)
        c.set_option("schwarz_dedupe", 1)
        c.close()


# ---- 2. stacked extension solves under multi_ch ------------------------------------------------------------------------------
MULTI_CASES = [("laplace", 10, 27), ("laplace", 8, 8), ("linelas", 8, 8)]      # (problem, cells per direction, nodes per box)
MULTI_CELLS = 8                                                                # coarse cells: a 2 x 2 x 2 lattice on mesh planes
_MULTI_REF = {}


def _multi_system(L, c, kind, M):
    m = L.structured_mesh(3, 1, M)
    c.mesh_set_dict(m)
    om = oracle_mesh(m)
    if kind == "laplace":
        c.pattern_build(1, L.BLOCK_SCALAR)
        c.assemble(L.FORM_LAPLACE)
        c.assemble_rhs([1.0])
        c.dirichlet([1, 2, 3], [0.0, 0.0, 0.0])
        return m, om, 1
    mu, nu = 2.0e6, 0.4
    c.pattern_build(3, L.BLOCK_FULL)
    c.assemble(L.FORM_LINELAS, [2.0 * mu * nu / (1.0 - 2.0 * nu), mu])
    c.assemble_rhs([0.0, 1.0, 0.0])
    c.dirichlet([2], [0.0, 0.0, 0.0])
    return m, om, 3


def _multi_reference(m, om, kind, M, target, reduced):
    key = (kind, M, target, reduced)
    if key not in _MULTI_REF:
        if kind == "laplace":
            A_bc, _, _, _, flags = fo.laplace_problem(om)
            is_dir, dofs = np.isin(flags, (1, 2, 3)), 1
        else:
            A_bc, _, _, _, flags = fo.linelas_problem(om, 2.0e6, 0.4)
            is_dir, dofs = fo.dirichlet_rows(flags, (2,), dofs=3), 3
        co = fo.CoarseGDSW(A_bc, m["conn"], m["xyz"], is_dir, dofs, cells_target=MULTI_CELLS, reduced=reduced)
        node_bin, nb, _ = fo.schwarz_bins(m["xyz"], target)
        ras = fo.RAS(A_bc, node_bin, nb, dofs=dofs)
        r = np.random.default_rng(5).standard_normal(A_bc.shape[0])
        _MULTI_REF[key] = (nb, ras.max_size, co.K0inv, r, ras.apply(r) + co.apply(r))
    return _MULTI_REF[key]


def test_multi_ch_cases_put_the_largest_box_on_both_sides_of_a_flight(fedd_lib):
    """The flights of k_apply_multi<RT, AM_CH> are 4 AM_CH = 16, 32, 64 columns long; the largest box of the three cases of
    test_stacked_extension_solves_under_multi_ch has 101, 46 and 138 dofs: three different remainders mod 64 (37, 46, 10), below
    and above a multiple of 16 (96 < 101 < 112, 32 < 46 < 48, 128 < 138 < 144), of 32 (96 < 101, 46 < 64, 128 < 138) and of 64
    (101 and 138 past one, 46 short of one), so a last flight is short by 10, 18 and 27 (of 32) and by 18, 27 and 54 (of 64)
    columns whose ids are read past the list's end."""
    L = fedd_lib
    c = L.Context(device=0)
    try:
        sizes = []
        for kind, M, target in MULTI_CASES:
            _multi_system(L, c, kind, M)
            c.schwarz_set_target(target, 1.0)
            c.schwarz_setup(1, L.COMBINE_RESTRICTED)
            sizes.append(c.schwarz_info()["max_size"])
        print("largest boxes:", sizes, "mod 64:", [s % 64 for s in sizes])
        assert len({s % 64 for s in sizes}) == 3
        assert max(sizes) > 128 and min(sizes) < 64
    finally:
        c.close()


@pytest.mark.parametrize("coarse", ["gdsw", "rgdsw"])
@pytest.mark.parametrize("kind,M,target", MULTI_CASES, ids=["%s-%d-%d" % s for s in MULTI_CASES])
def test_stacked_extension_solves_under_multi_ch(fedd_lib, kind, M, target, coarse):
    """multi_ch 4 (default), 8 and 16: k_apply_multi<RT, 4 | 8 | 16> in the stacked extension solves of the GDSW / RGDSW setup
    (gdsw_block 1, sixteen columns at a time, driven to 1e-13).  RT by the owned dofs of the largest box: 27 and 8 (Laplace) and 24
    (elasticity): RT = 2 in all three cases; the columns are 101, 46 and 138.  K0^-1 (fedd_schwarz_coarse_get) and one two-level
    apply against fo.CoarseGDSW + fo.RAS at the 1e-10 of test_gpu_two_level, and between the three values at 1e-11.  (The
    flights only group the gathers: the matrix-core steps run in the same order for every AM_CH, but the extension solves
    around them are iterative, so nothing here is asserted bitwise.  Nor can these comparisons see whether the entries of R
    gathered through ids past the list's end are dropped: such a column meets an entry of the inverse that the kernel has
    already set to zero, and the ids past the end are dof 0, whose entry of R is finite.)
    Measured: Laplace K0^-1 1.1e-15 and the apply 1.6e-14 at most; elasticity K0^-1 1.0e-14 and the apply 6.6e-11 of max |z| (of
    the 1e-10 allowed; the same figure for the three values); multi_ch 8 and 16 against 4: no bit differs, in all six cases."""
    L = fedd_lib
    c = L.Context(device=0)
    try:
        m, om, dofs = _multi_system(L, c, kind, M)
        reduced = coarse == "rgdsw"
        nb, max_size, K0inv, r, zo = _multi_reference(m, om, kind, M, target, reduced)
        c.schwarz_set_target(target, 1.0)
        c.schwarz_set_coarse(MULTI_CELLS)
        c.set_option("gdsw_tol", 1e-13)
        c.set_option("gdsw_block", 1)
        out = {}
        for ch in (4, 8, 16):
            c.set_option("multi_ch", ch)
            c.schwarz_setup(1, L.COMBINE_RESTRICTED, two_level=1, coarse_kind=L.COARSE_RGDSW if reduced else L.COARSE_GDSW)
            info = c.schwarz_info()
            assert info["n_subdomains"] == nb and info["max_size"] == max_size
            Kinv = c.schwarz_coarse()[1]
            z = c.schwarz_apply(r)
            out[ch] = (Kinv, z)
            assert Kinv.shape == K0inv.shape
            print("%s M %d target %d %s multi_ch %d: largest box %d; K0^-1 %.2e, apply %.2e" % (
                kind, M, target, coarse, ch, info["max_size"], np.abs(Kinv - K0inv).max() / np.abs(K0inv).max(),
                np.abs(z - zo).max() / np.abs(zo).max()))
            np.testing.assert_allclose(Kinv, K0inv, rtol=0, atol=1e-10 * np.abs(K0inv).max(), err_msg="multi_ch %d" % ch)
            np.testing.assert_allclose(z, zo, rtol=0, atol=1e-10 * np.abs(zo).max(), err_msg="multi_ch %d" % ch)
        for ch in (8, 16):
            print("    multi_ch %d against 4: K0^-1 %.2e, apply %.2e" % (
                ch, np.abs(out[ch][0] - out[4][0]).max() / np.abs(K0inv).max(), np.abs(out[ch][1] - out[4][1]).max() / np.abs(zo).max()))
            np.testing.assert_allclose(out[ch][0], out[4][0], rtol=0, atol=1e-11 * np.abs(K0inv).max())
            np.testing.assert_allclose(out[ch][1], out[4][1], rtol=0, atol=1e-11 * np.abs(zo).max())
    finally:
        c.set_option("multi_ch", 4)
        c.set_option("gdsw_tol", 0.0)
        c.set_option("gdsw_block", 1)
        c.close()


# ---- 3. block dot products under forced column-group counts ------------------------------------------------------------------
DOT_M = 16
DOT_RTOL = 1e-10
DOT_MIN_ITS = 64        # a cycle of this many iterations has a block with k + sa >= 65 columns: 33 column groups of two
_DOT_REF = {}


def _dot_system(L, c):
    """unpreconditioned 3D Laplace, 16^3 cells, with a right-hand side that excites every mode (the assembled f = 1 plus 0.3 of
    its size of seeded noise): 69 iterations to 1e-10 in the oracle's GMRES, against 43 for f = 1 alone"""
    m, om, A_bc, rhs_bc = _setup_laplace(L, c, 3, DOT_M)
    if "b" not in _DOT_REF:
        b = rhs_bc + 0.3 * np.abs(rhs_bc).max() * np.random.default_rng(DOT_M).standard_normal(rhs_bc.shape[0])
        _DOT_REF["b"] = b
        _DOT_REF["xd"] = fo.direct_solve(A_bc, b)
    return read_back(c), _DOT_REF["b"], _DOT_REF["xd"]


def _relres(A, b, x):
    return float(np.linalg.norm(b - A @ x) / np.linalg.norm(b))


@pytest.mark.parametrize("s,fuse", [(4, -1), (8, -1), (16, 0), (16, 1)])
def test_block_dot_under_forced_column_groups(fedd_lib, s, fuse):
    """k_blockdot<S, 2, SS_CG> of the s-step solver (gmres_kind 2) with gmres_dot_gy 0 (automatic: 5 row blocks of 1024 rows ->
    min(4, 205) = 4 grid rows), 1, 2, 3, 5, 8 grid rows; restart 100, rtol 1e-10 (the blocks themselves are then at most 5 long:
    gmres_tol_blocks).  Instantiations: gmres_s 4 -> <4, 2, 4>, 8 -> <8, 2, 4>, 16 -> <16, 2, 2>.  One workgroup walks
    ceil(ncg / gy) column groups, ncg = ceil((k + sa) / SS_CG); its wave totals are parked in LDS for SS_LDS_GROUPS = 32 groups
    and flushed in mid-loop only beyond.  With SS_CG = 4 a cycle of 100 vectors has at most 26 groups: <4, 2, 4> and <8, 2, 4>
    cannot reach the mid-loop flush at restart 100 (they are run for the stride and the prefetch at gy 1, 2, 3, 5, 8).
    <16, 2, 2> reaches it with gy = 1 once a cycle holds 64 iterations (k + sa >= 65: 33 groups); asserted: at least 64
    iterations in the first cycle.  With gmres_fuse 1 the second dot of a block runs inside k_blockfuse, the first one stays
    k_blockdot.
    Against the run at gy = 0: iterations equal within 1, cut_blocks equal, fused_blocks = blocks (fuse 1) or 0; true residual
    from the matrix read back <= rtol; x against fo.direct_solve at RTOL max |x|.
    Measured: 69 iterations in every one of the 24 runs (18 blocks at s = 4, 14 at 8 and 16, none cut), true residual 7.02e-11,
    x 1.98e-11 of max |x| from the direct solve."""
    L = fedd_lib
    c = L.Context(device=0)
    try:
        A, b, xd = _dot_system(L, c)
        c.set_option("gmres_kind", 2)
        c.set_option("gmres_s", s)
        c.set_option("gmres_fuse", fuse)
        ref = None
        for gy in (0, 1, 2, 3, 5, 8):
            c.set_option("gmres_dot_gy", gy)
            x, its, rel = c.gmres(b, rtol=DOT_RTOL, max_it=400, restart=100, use_prec=False)
            info = c.gmres_info()
            tr = _relres(A, b, x)
            err = float(np.abs(x - xd).max() / np.abs(xd).max())
            print("s %d fuse %d gy %d: %d iterations, %s, true residual %.3e, error %.2e" % (s, fuse, gy, its, info, tr, err))
            assert info["kind"] == 2 and info["s"] == s
            if ref is None:
                ref = (its, info)
            assert abs(its - ref[0]) <= 1, (gy, its, ref[0])
            assert info["cut_blocks"] == ref[1]["cut_blocks"], (gy, info, ref[1])
            assert info["fused_blocks"] == (info["blocks"] if (s > 8 and fuse == 1) else 0), (gy, info)
            if s > 8:
                assert its >= DOT_MIN_ITS, its        # one workgroup (gy = 1) walked more than 32 column groups
            assert rel <= DOT_RTOL and tr <= DOT_RTOL, (gy, rel, tr)
            np.testing.assert_allclose(x, xd, rtol=0, atol=RTOL * np.abs(xd).max(), err_msg="gmres_dot_gy %d" % gy)
    finally:
        c.set_option("gmres_dot_gy", 0)
        c.set_option("gmres_fuse", -1)
        c.set_option("gmres_s", 0)
        c.set_option("gmres_kind", 2)
        c.close()


def test_two_vector_dot_under_forced_column_groups(fedd_lib):
    """k_multidot2<4> of the DCGS2 solver (gmres_kind 0; 1 is the two-pass CGS2 on k_multidot) with md2_gy 0, 1, 2, 3, 64 on the
    system of test_block_dot_under_forced_column_groups.  3 row blocks of 2048 rows: the automatic value is 683, so by default the
    launch takes min(683, ncg) = ncg grid rows (ncg = ceil((k + 2) / 8) <= 13) and no workgroup ever strides; 1, 2, 3 make it
    walk up to 13, 7, 5 groups of eight columns, and 64 > ncg is cut by the min like the default.
    Against the run at md2_gy 0: iterations equal within 1; true residual from the matrix read back <= rtol; x against
    fo.direct_solve at RTOL max |x|.  (Blocks, cut and fused blocks are counters of the s-step solver.)
    Measured: 69 iterations, true residual 7.02e-11, x 1.98e-11 of max |x| from the direct solve, for all five values."""
    L = fedd_lib
    c = L.Context(device=0)
    try:
        A, b, xd = _dot_system(L, c)
        c.set_option("gmres_kind", 0)
        its0 = None
        for gy in (0, 1, 2, 3, 64):
            c.set_option("md2_gy", gy)
            x, its, rel = c.gmres(b, rtol=DOT_RTOL, max_it=400, restart=100, use_prec=False)
            tr = _relres(A, b, x)
            err = float(np.abs(x - xd).max() / np.abs(xd).max())
            print("md2_gy %d: %d iterations, true residual %.3e, error %.2e" % (gy, its, tr, err))
            if its0 is None:
                its0 = its
            assert abs(its - its0) <= 1 and its > 16, (gy, its, its0)      # (more than two column groups: a stride to take)
            assert rel <= DOT_RTOL and tr <= DOT_RTOL, (gy, rel, tr)
            np.testing.assert_allclose(x, xd, rtol=0, atol=RTOL * np.abs(xd).max(), err_msg="md2_gy %d" % gy)
    finally:
        c.set_option("md2_gy", 0)
        c.set_option("gmres_kind", 2)
        c.close()


# ---- 4. small companions -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,M", [(3, 15), (2, 63)])
def test_assembly_under_forced_lds_budgets(fedd_lib, dim, M):
    """asm_lds_kb 2, 4, 8, 37 (default): rows per workgroup R = min(63, budget / per_row) of the row-major assembly kernels, which
    P1 Laplace and elasticity take with asm_tiles 0 (the element-major tiles of the default do not read the option): Laplace the
    pair sweep (launch_pairs, per_row = 12 x contributions), elasticity on FULL blocks the slot-addressed kernel (launch_slots).
    Distorted lattice (no two elements alike), 4096 nodes: R = 1 ... 32 in 3D and 9 ... 63 in 2D for Laplace, fewer for
    elasticity; 4096 is a multiple of none of the odd R, so the last workgroup's rows are cut.  Pattern and values against the
    oracle (assert_matrix_close, RTOL of the row scale), and the values bit for bit those of the default budget: a row's
    contributions are summed in the same order whatever rows share its workgroup.
    Measured: 6.8e-16 (3D Laplace), 7.7e-16 (3D elasticity), 4.4e-16 and 5.7e-16 (2D) of the row scale; bit-identical across
    the four budgets in all four cases."""
    L = fedd_lib
    c = L.Context(device=0)
    try:
        m = distorted(L.structured_mesh(dim, 1, M), 0.15, "all", seed=1)
        check_mesh(m, 0.8)
        om = oracle_mesh(m)
        n = om.n_global
        c.mesh_set_dict(m)
        c.set_option("asm_tiles", 0)
        mu, nu = 2.0e6, 0.4
        lam = 2.0 * mu * nu / (1.0 - 2.0 * nu)
        forms = (("laplace", 1, L.BLOCK_SCALAR, L.FORM_LAPLACE, None, fo.assembly_laplace(om)),
                 ("linelas", dim, L.BLOCK_FULL, L.FORM_LINELAS, [lam, mu], fo.assembly_linelas(om, lam, mu)))
        for name, dofs, mode, form, params, A_o in forms:
            c.pattern_build(dofs, mode)
            vals = {}
            for kb in (37, 2, 4, 8):
                c.set_option("asm_lds_kb", kb)
                c.assemble(form, params)
                err = assert_matrix_close(csr_global(c, dofs * n)[0], A_o)
                vals[kb] = c.csr_get()[2].copy()
                print("dim %d %s asm_lds_kb %d: error %.2e of the row scale, bits equal to the default %s"
                      % (dim, name, kb, err, np.array_equal(vals[kb], vals[37])))
            for kb in (2, 4, 8):
                assert np.array_equal(vals[kb], vals[37]), (name, kb, np.count_nonzero(vals[kb] != vals[37]))
    finally:
        c.set_option("asm_lds_kb", 37)
        c.set_option("asm_tiles", 1)
        c.close()


@pytest.mark.parametrize("exact_public", [0, 1])
def test_spmv_with_and_without_the_non_temporal_stream(fedd_lib, exact_public):
    """spmv_nt -1 (by size: off at this size), 0 and 1 on the 13^3-cell Laplace system of test_spmv_kernels_agree: k_spmv_win<false>
    and <true> on the solver's compacted stream (spmv_exact_public 0) and on the parity CSR (1).  The same bits, and every row
    within the rounding bound of its extended-precision sum (test_gpu_distorted._spmv_exact_check).
    Measured: the three values agree in every bit, on both streams; no row outside its bound."""
    L = fedd_lib
    c = L.Context(device=0)
    try:
        _setup_laplace(L, c, 3, 13)
        rowptr, col, val, _ = c.csr_get()
        x = np.random.default_rng(11).standard_normal(rowptr.shape[0] - 1)
        c.set_option("spmv_exact_public", exact_public)
        ys = {}
        for nt in (-1, 0, 1):
            c.set_option("spmv_nt", nt)
            ys[nt] = c.spmv(x)
            _spmv_exact_check(rowptr, col, val, x, ys[nt])
        assert np.array_equal(ys[0], ys[-1]) and np.array_equal(ys[1], ys[0])
    finally:
        c.set_option("spmv_nt", -1)
        c.set_option("spmv_exact_public", 1)
        c.close()

"""The class SpMV wave by wave (spmv.hip: k_spmv_cls, k_spmv_cls_lds, cls_row, cls_row_fixed) against a statement of its contract
that lives outside the library.

The contract of the solver's product: per row the entries with not (|a_ij| <= 2^-52 max_k |a_ik|), in CSR order, every product
rounded on its own and added to the running sum (s = s + (a_ij * x_j), s starting at 0.0, nothing fused).  host_product below
is that statement in numpy -- float64 elementwise multiply and add are IEEE and unfused --, and the three device paths (the
per-entry kernel, the class kernel on the table, the class kernel with its block's values in LDS) have to give its bits.

What a row runs through in the class kernels is decided per wave of 64 consecutive rows (both in the 1024-row blocks of the
strides 8 / 16 and in the 512-row blocks of stride 48), so wave_census classifies the 64-aligned groups of rows of the kept
structure, and every case asserts that it reaches the kinds it is there for BEFORE it looks at y:

    (a) one pattern, 7 entries, middle offsets d - 1, d, d + 1     cls_row_fixed<7, true>, x from the neighbouring lanes
    (b) the same with 5 entries                                    cls_row_fixed<5, true>, x from the neighbouring lanes
    (c) one pattern, 7 or 5 entries, middle offsets not in a run   cls_row_fixed, every x loaded
    (d) 7 or 5 entries in every row, several patterns              cls_row_fixed, every x loaded
    (e) one pattern, 6 or 4 entries                                the predicated form
    (f) rows of several lengths                                    the predicated form
    (g) the partial last wave                                      (rows past the end inactive: no exchange)
    (h) every other wave of one length (1: a line of Dirichlet rows; 6 or 4 with several patterns; ...): the predicated form

Lattices (structured_mesh with per-direction cells; scalar Laplace; "neumann" = no dirichlet call at all):

    A  3D 128 x 4 x 4 cells, h = 1/4: exact arithmetic, one class per pattern, every block on the LDS path
    B  3D 130 x 3 x 3 cells, h = 1/3: rounded values, many classes; the cap forced low puts kind-(a) waves into flagged blocks
    C  2D 128 x 8 cells, h = 1/8: the 5-entry exchange and the 4-entry rows of a Neumann edge
    D  A with the nodes of two x-lines interleaved: x-neighbours two rows apart, kinds (c) / (d) at 7 entries
    E  the cube of 66 cells per side under the default gates (no forced dictionary): the only case above a few thousand rows
"""
import math

import numpy as np
import pytest

from test_gpu_spmv_cls_lds import LOW_CAPS

pytestmark = pytest.mark.gpu

WAVE = 64
BLOCK_ROWS = 1024       # rows per workgroup of the class kernels at table stride 8
LDS_CAP_8 = 160         # classes a block's list holds at table stride 8


# ---- host side: the contract and the census (numpy only) --------------------------------------------------------------------

def padded_sum(V, X, klen):
    """s = s + (v_j * x_j) column position by column position over the padded rows: two separate float64 operations per entry"""
    s = np.zeros(V.shape[0])
    for j in range(V.shape[1]):
        p = V[:, j] * X[:, j]
        s = np.where(j < klen, s + p, s)
    return s


def _two_prod(a, b):
    """a * b = p + e exactly (Veltkamp split, Dekker product; no overflow or underflow at the magnitudes of these tests)"""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def exact_sum(V, X, klen):
    """the same kept entries summed in np.longdouble where that is wider than float64, else math.fsum over exact products"""
    n, L = V.shape
    if np.finfo(np.longdouble).nmant > 52:
        s = np.zeros(n, dtype=np.longdouble)
        for j in range(L):
            s = s + np.where(j < klen, V[:, j].astype(np.longdouble) * X[:, j].astype(np.longdouble), np.longdouble(0))
        return s
    p, e = _two_prod(np.where(np.arange(L)[None, :] < klen[:, None], V, 0.0), X)
    return np.array([math.fsum(np.concatenate([p[i], e[i]])) for i in range(n)])


def host_product(rowptr, col, val, x, tol=2.0 ** -52):
    """(y_host, kept, y_exact) of the CSR ctx.csr_get() returns: the kernel's drop rule, the kept entries padded to the longest
    row, products and sums separate and in entry order.  kept: rowptr / col / val of the kept entries, len per row, and the
    padded V (values) and C (columns)."""
    n = rowptr.shape[0] - 1
    row_of = np.repeat(np.arange(n), np.diff(rowptr))
    rowmax = np.zeros(n)
    np.maximum.at(rowmax, row_of, np.abs(val))
    keep = ~(np.abs(val) <= tol * rowmax[row_of])
    krow, kcol, kval = row_of[keep], col[keep].astype(np.int64), val[keep]
    klen = np.bincount(krow, minlength=n)
    kptr = np.concatenate([[0], np.cumsum(klen)])
    L = max(int(klen.max()), 1)
    pos = np.arange(kval.shape[0]) - kptr[krow]
    V = np.zeros((n, L))
    C = np.zeros((n, L), dtype=np.int64)
    V[krow, pos] = kval
    C[krow, pos] = kcol
    X = x[C]
    kept = dict(rowptr=kptr, col=kcol, val=kval, len=klen, V=V, C=C)
    return padded_sum(V, X, klen), kept, exact_sum(V, X, klen)


def wave_census(kept_rowptr, kept_col, n):
    """(counts, waves): every 64-aligned group of rows classified as in the module docstring.  counts: kind -> waves; waves: a
    list of (kind, first row, end row, entries per row -- 0 where the rows differ in length)."""
    klen = np.diff(kept_rowptr)
    L = max(int(klen.max()), 1)
    row_of = np.repeat(np.arange(n), klen)
    pos = np.arange(kept_col.shape[0]) - kept_rowptr[row_of]
    off = np.full((n, L), np.iinfo(np.int64).min)      # (the padding is the same in every row of a length)
    off[row_of, pos] = kept_col - row_of
    waves = []
    for r0 in range(0, n, WAVE):
        r1 = min(r0 + WAVE, n)
        ln = klen[r0:r1]
        length = int(ln[0]) if np.all(ln == ln[0]) else 0
        if r1 - r0 < WAVE:
            kind = "g"
        elif length == 0:
            kind = "f"
        else:
            one = bool(np.all(off[r0:r1] == off[r0]))
            if length in (7, 5):
                c = length // 2
                d = off[r0]
                kind = "d" if not one else ("ab"[length == 5] if d[c - 1] + 1 == d[c] and d[c] + 1 == d[c + 1] else "c")
            else:
                kind = "e" if one and length in (6, 4) else "h"
        waves.append((kind, r0, r1, length))
    return {k: sum(1 for w in waves if w[0] == k) for k in "abcdefgh"}, waves


def of_kind(waves, kind, length=None):
    return [w for w in waves if w[0] in kind and (length is None or w[3] == length)]


def row_keys(kept, n):
    """per row (length | offsets | value bits), the padding zero: rows with the same first 1 + L columns share a column
    pattern, rows with the same key a class"""
    L = kept["C"].shape[1]
    key = np.concatenate([kept["len"][:, None], kept["C"] - np.arange(n)[:, None], kept["V"].view(np.int64)], axis=1)
    key[:, 1:1 + L][np.arange(L)[None, :] >= kept["len"][:, None]] = 0
    return key


def classes_per_block(kept, n):
    """bitwise-distinct (length, offsets, values) rows per 1024-row block: the classes a block's list has to hold"""
    key = row_keys(kept, n)
    return np.array([np.unique(key[b:b + BLOCK_ROWS], axis=0).shape[0] for b in range(0, n, BLOCK_ROWS)])


# ---- device side --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx(fedd_lib):
    c = fedd_lib.Context(device=0)
    yield c
    c.close()


def restore(c):
    for key, v in (("spmv_cls_lds", 1), ("spmv_cls_lds_cap", 0), ("spmv_pattern", 1), ("spmv_exact_public", 1), ("gmres_s", 0)):
        c.set_option(key, v)


LATTICES = {"A": (3, [128, 4, 4], [32.0, 1.0, 1.0], 3225),
            "B": (3, [130, 3, 3], [130.0 / 3.0, 1.0, 1.0], 2096),
            "C": (2, [128, 8], [16.0, 1.0], 1161)}
BOUNDARIES = {"dirichlet": (1, 2, 3), "neumann": ()}


def lattice(L, name):
    dim, cells, size, rows = LATTICES[name]
    m = L.structured_mesh(dim, 1, cells, size=size)
    assert m["xyz"].shape[0] == rows
    return m


def interleaved(m, nx, pairs):
    """the mesh with the nodes of the x-lines (a, b) of every pair interleaved -- new id 2 i + {0, 1} within the pair --, the
    lines in no pair behind them; perm[new] = old"""
    n = m["xyz"].shape[0]
    i = np.arange(nx)
    perm = [np.stack([a * nx + i, b * nx + i], axis=1).ravel() for a, b in pairs]
    paired = {l for p in pairs for l in p}
    perm += [l * nx + i for l in range(n // nx) if l not in paired]
    perm = np.concatenate(perm)
    assert np.array_equal(np.sort(perm), np.arange(n))
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    m2 = dict(m)
    m2["xyz"] = m["xyz"][perm]
    for key in ("gid_rep", "flag_rep", "gid_uni", "flag_uni"):
        m2[key] = m[key][perm]
    m2["conn"] = inv[m["conn"]].astype(m["conn"].dtype)
    return m2


class Case:
    """a system assembled on the context, its host product and its census"""

    def __init__(self, L, c, name, mesh, flags, seed):
        c.mesh_set_dict(mesh)
        c.pattern_build(1, L.BLOCK_SCALAR)
        c.assemble(L.FORM_LAPLACE)
        c.assemble_rhs([1.0])
        if flags:
            c.dirichlet(list(flags), [0.0] * len(flags))
        self.name = name
        self.n, n_cols, _ = c.csr_sizes()
        assert n_cols == self.n
        rowptr, col, val, _ = c.csr_get()
        rng = np.random.default_rng(seed)
        # (scaled entry by entry over 40 binades: a neighbour's value taken from the wrong place cannot hide in the rounding)
        self.x = rng.standard_normal(self.n) * 2.0 ** rng.integers(-20, 21, self.n)
        self.y_host, self.kept, self.y_exact = host_product(rowptr, col, val, self.x)
        self.counts, self.waves = wave_census(self.kept["rowptr"], self.kept["col"], self.n)
        self.nblk = -(-self.n // BLOCK_ROWS)
        # (the dictionary holds 64 column patterns; with no more than that every row finds its own and joins a class)
        self.n_patterns = np.unique(row_keys(self.kept, self.n)[:, :1 + self.kept["C"].shape[1]], axis=0).shape[0]
        by_len = {}
        for kind, _, _, length in self.waves:
            by_len[(kind, length)] = by_len.get((kind, length), 0) + 1
        print("%s: %d rows, %d blocks, %d column patterns, rows of %s entries; waves %s; (kind, entries): %s"
              % (name, self.n, self.nblk, self.n_patterns, sorted(set(self.kept["len"].tolist())), self.counts, sorted(by_len.items())))

    def reaches(self, kind, length=None):
        return len(of_kind(self.waves, kind, length))


def assert_bits(case, y, label):
    """np.array_equal(y, y_host), and where it fails: which rows, in waves of which kind"""
    bad = np.nonzero(~((y == case.y_host) | (np.isnan(y) & np.isnan(case.y_host))))[0]
    if bad.shape[0]:
        kinds = sorted({(case.waves[r // WAVE][0], case.waves[r // WAVE][3]) for r in bad.tolist()})
        rel = np.abs(y[bad] - case.y_host[bad]) / np.maximum(np.abs(case.y_host[bad]), 1e-300)
        pytest.fail("%s, %s: %d rows differ from the host product, first %s (lanes %s), in waves of (kind, entries) %s; largest relative "
                    "difference %.3e" % (case.name, label, bad.shape[0], bad[:8].tolist(), (bad[:8] % WAVE).tolist(), kinds, rel.max()))
    assert np.array_equal(y, case.y_host)


def check_host_helper(case):
    """the host statement itself against the exact sum of the same entries: any summation order of len_i products stays within
    len_i 2^-52 (|A| |x|)_i of it (the bound derived in test_gpu_spmv_launch_table.py)"""
    k = case.kept
    bound = k["len"] * 2.0 ** -52 * padded_sum(np.abs(k["V"]), np.abs(case.x[k["C"]]), k["len"])
    err = np.abs((case.y_host.astype(case.y_exact.dtype) - case.y_exact).astype(np.float64))
    print("%s: host product against the exact sum: largest error / bound %.3f" % (case.name, float(np.max(err / np.maximum(bound, 1e-300)))))
    assert np.all(err <= bound)
    assert np.abs(case.y_host).max() > 0


def product(c, x, lds, cap=0):
    c.set_option("spmv_cls_lds", lds)
    c.set_option("spmv_cls_lds_cap", cap)
    return c.spmv(x), c.spmv_info()


def check_device_paths(c, case, pattern, all_lds=False):
    """the three device paths against the host product; returns the info of the LDS path.  Call with spmv_exact_public 0."""
    c.set_option("spmv_pattern", pattern)
    y0, info0 = product(c, case.x, 0)
    assert info0["row_classes"] >= 1 and info0["column_patterns"] >= 1, info0
    assert info0["class_blocks_lds"] == 0 and info0["class_blocks_fallback"] == 0, info0
    assert_bits(case, y0, "spmv_cls_lds 0")
    y1, info1 = product(c, case.x, 1)
    print("%s: spmv_cls_lds 1: %s" % (case.name, info1))
    assert info1["row_classes"] == info0["row_classes"] and info1["rows_in_classes"] == info0["rows_in_classes"]
    assert info1["class_blocks_lds"] >= 1 and info1["class_blocks_lds"] + info1["class_blocks_fallback"] == case.nblk, info1
    if all_lds:
        assert info1["class_blocks_fallback"] == 0, info1
    assert_bits(case, y1, "spmv_cls_lds 1")
    c.set_option("spmv_pattern", 0)
    ye = c.spmv(case.x)
    infoe = c.spmv_info()
    assert infoe["column_patterns"] == 0 and infoe["row_classes"] == 0, infoe
    assert_bits(case, ye, "spmv_pattern 0")
    c.set_option("spmv_pattern", pattern)
    return y1, info1


def check_planted_edge_lanes(case, y, kind, length):
    """of the census, not of the kernel: in one wave of the kind, the host product with the outer x of lanes 0 and 63 swapped
    differs from y in just these two rows -- this x would show an edge-lane error"""
    _, r0, r1, _ = of_kind(case.waves, kind, length)[0]
    k, c = case.kept, length // 2
    X = case.x[k["C"][r0:r1]]
    X[0, c - 1], X[WAVE - 1, c + 1] = X[WAVE - 1, c + 1], X[0, c - 1]
    yp = padded_sum(k["V"][r0:r1], X, k["len"][r0:r1])
    assert yp[0] != y[r0] and yp[WAVE - 1] != y[r1 - 1]
    assert np.array_equal(yp[1:WAVE - 1], y[r0 + 1:r1 - 1])




# ---- the helpers themselves, on rows written by hand ----------------------------------------------------------------------------

def test_host_helpers_on_rows_written_by_hand():
    """drop rule, entry order and every kind of the census on a matrix that can be checked by eye: wave w of 64 rows has the
    offsets HAND[w] (columns shifted by 16, so no row leaves the matrix); no device involved"""
    tiny = 2.0 ** -52 * 1.75        # (1.75 is the largest entry of the rows below: offsets +-3)
    HAND = [("b", (-3, -1, 0, 1, 3)), ("a", (-9, -3, -1, 0, 1, 3, 9)), ("c", (-3, -2, 0, 2, 3)), ("d", ((-3, -1, 0, 1, 3), (-4, -1, 0, 1, 3))),
            ("e", (-3, -1, 0, 1)), ("f", ((-1, 0, 1), (0,))), ("h", (0,)), ("e", (-3, -1, 0, 1, 3, 5)), ("g", (-1, 0))]
    n = 8 * WAVE + 3
    rows, cols, vals = [], [], []
    for r in range(n):
        offs = HAND[r // WAVE][1]
        offs = offs[r % 2] if isinstance(offs[0], tuple) else offs
        for o in offs:
            rows.append(r)
            cols.append(r + 16 + o)
            # wave 7: its sixth entry lies just above the drop threshold and stays
            vals.append(np.nextafter(tiny, 1.0) if o == 5 else 1.0 + 0.25 * abs(o))
        if r < WAVE:        # wave 0: an entry AT the threshold goes
            rows.append(r)
            cols.append(r + 16 + 5)
            vals.append(-tiny)
    rows, cols, vals = np.array(rows), np.array(cols, dtype=np.int32), np.array(vals)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    x = np.random.default_rng(3).standard_normal(n + 32)
    y, kept, ye = host_product(rowptr, cols, vals, x)
    assert kept["val"].shape[0] == vals.shape[0] - WAVE and kept["len"][:WAVE].tolist() == [5] * WAVE and kept["len"][7 * WAVE] == 6
    ref = np.zeros(n)
    for r, c, v in zip(rows.tolist(), cols.tolist(), vals.tolist()):    # (entry by entry, Python floats: IEEE double, unfused)
        if v != -tiny:
            ref[r] = ref[r] + v * x[c]
    assert np.array_equal(y, ref)
    assert np.all(np.abs((y.astype(ye.dtype) - ye).astype(np.float64)) <= kept["len"] * 2.0 ** -52 * padded_sum(np.abs(kept["V"]), np.abs(x[kept["C"]]), kept["len"]))
    counts, waves = wave_census(kept["rowptr"], kept["col"], n)
    assert [w[0] for w in waves] == [h[0] for h in HAND], waves
    assert [w[3] for w in waves] == [5, 7, 5, 5, 4, 0, 1, 6, 2] and waves[-1][1:3] == (8 * WAVE, n)
    assert counts == {"a": 1, "b": 1, "c": 1, "d": 1, "e": 2, "f": 1, "g": 1, "h": 1}


# ---- the lattices ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("boundary", list(BOUNDARIES))
def test_lattice_a_exact_arithmetic_every_block_on_the_lds_path(fedd_lib, ctx, boundary):
    """7-entry waves whose x comes from the neighbouring lanes, on the LDS path; with Neumann boundaries also the 5-entry waves of
    an x-edge with (b) and without (c) consecutive middle offsets and the 6-entry waves of a face (e)"""
    case = Case(fedd_lib, ctx, "A " + boundary, lattice(fedd_lib, "A"), BOUNDARIES[boundary], 4101)
    if boundary == "dirichlet":
        assert case.reaches("a", 7) >= 1 and case.reaches("f") >= 1, case.counts
    else:
        assert case.reaches("a", 7) >= 1 and case.reaches("b", 5) >= 1 and case.reaches("e", 6) >= 1 and case.reaches("c", 5) >= 1, case.counts
    assert case.nblk == 4 and case.n % BLOCK_ROWS != 0 and case.kept["len"].max() <= 8 and case.n_patterns <= 64
    check_host_helper(case)
    try:
        ctx.set_option("spmv_exact_public", 0)      # fedd_spmv = the solver's stream
        y, info = check_device_paths(ctx, case, 2, all_lds=True)
        # h = 1/4: the arithmetic is exact, one class per (pattern, Dirichlet or not), every row in one
        assert info["rows_in_classes"] == case.n and info["row_classes"] <= 2 * info["column_patterns"], info
        check_planted_edge_lanes(case, y, "a", 7)
    finally:
        restore(ctx)


@pytest.mark.parametrize("boundary", list(BOUNDARIES))
def test_lattice_b_rounded_values_and_flagged_blocks(fedd_lib, ctx, boundary):
    """h = 1/3: the rows differ in their last bits, a block holds dozens of classes.  Default cap, then the cap forced low: a
    launch with listed and flagged blocks in which a flagged block holds a kind-(a) wave -- cls_row<8, false>, length-uniform
    without the exchange.  Which blocks a cap flags is counted on the host: the bitwise-distinct rows of the block."""
    case = Case(fedd_lib, ctx, "B " + boundary, lattice(fedd_lib, "B"), BOUNDARIES[boundary], 4102)
    assert case.reaches("a", 7) >= 1, case.counts
    assert case.kept["len"].max() <= 8 and case.n_patterns <= 64       # table stride 8; every row finds its pattern in the dictionary
    check_host_helper(case)
    need = classes_per_block(case.kept, case.n)
    blocks_a = sorted({w[1] // BLOCK_ROWS for w in of_kind(case.waves, "a", 7)})
    print("%s: classes per block %s, kind-(a) waves in blocks %s" % (case.name, need.tolist(), blocks_a))
    try:
        ctx.set_option("spmv_exact_public", 0)
        y, info = check_device_paths(ctx, case, 2)
        assert info["rows_in_classes"] == case.n, info
        assert info["class_blocks_fallback"] == np.count_nonzero(need > LDS_CAP_8), (info, need)
        mixed = flagged_a = 0
        for cap in LOW_CAPS:
            yc, infoc = product(ctx, case.x, 1, cap)
            print("%s: cap %d: %d blocks with a list, %d flagged" % (case.name, cap, infoc["class_blocks_lds"], infoc["class_blocks_fallback"]))
            assert infoc["class_blocks_lds"] + infoc["class_blocks_fallback"] == case.nblk, (cap, infoc)
            assert infoc["class_blocks_fallback"] == np.count_nonzero(need > cap), (cap, infoc, need)
            assert_bits(case, yc, "spmv_cls_lds_cap %d" % cap)
            if infoc["class_blocks_lds"] >= 1 and infoc["class_blocks_fallback"] >= 1:
                mixed += 1
                flagged_a += 1 if any(need[b] > cap for b in blocks_a) else 0
        assert mixed >= 1 and flagged_a >= 1, (mixed, flagged_a)
        y2, info2 = product(ctx, case.x, 1)         # the default cap again: the lists are rebuilt for it
        assert np.array_equal(y2, y) and info2 == info
        check_planted_edge_lanes(case, y, "a", 7)
    finally:
        restore(ctx)


@pytest.mark.parametrize("boundary", list(BOUNDARIES))
def test_lattice_c_two_dimensions(fedd_lib, ctx, boundary):
    """the exchange with 5 entries (b); with Neumann boundaries the 4-entry rows of an edge (e)"""
    case = Case(fedd_lib, ctx, "C " + boundary, lattice(fedd_lib, "C"), BOUNDARIES[boundary], 4103)
    assert case.reaches("b", 5) >= 1, case.counts
    if boundary == "neumann":
        assert case.reaches("e", 4) >= 1, case.counts
    assert case.nblk == 2 and case.kept["len"].max() <= 8 and case.n_patterns <= 64
    check_host_helper(case)
    try:
        ctx.set_option("spmv_exact_public", 0)
        y, info = check_device_paths(ctx, case, 2)
        assert info["rows_in_classes"] == case.n, info
        check_planted_edge_lanes(case, y, "b", 5)
    finally:
        restore(ctx)


# lattice A's x-lines (line j + 5 k: 129 nodes) in pairs of lines that are no neighbours in y or z.  (6, 18) pairs two interior
# lines whose four neighbour lines are paired with each other in the same order: one pattern for both, x-neighbours at -2, +2
# (c).  (8, 16) pairs two interior lines whose neighbour lines sit elsewhere: the rows alternate between two patterns (d).  Line
# 24, an edge of the lattice, stays alone: Dirichlet rows, like its neighbour lines 19 and 23.
D_PAIRS = [(0, 12), (1, 13), (2, 14), (3, 15), (4, 20), (5, 17), (6, 18), (7, 19), (8, 16), (9, 21), (10, 22), (11, 23)]


def test_lattice_d_renumbered_x_neighbours_two_rows_apart(fedd_lib, ctx):
    """7-entry waves that are length-uniform but take no x from the neighbouring lanes: one pattern with middle offsets -2, 0, 2
    (c) and two patterns in turn (d), on the LDS path.  (Eight patterns, every row in a class: the cover gate stays as it is.)"""
    case = Case(fedd_lib, ctx, "D dirichlet", interleaved(lattice(fedd_lib, "A"), 129, D_PAIRS), BOUNDARIES["dirichlet"], 4104)
    print("%s: %d waves of kind (c), %d of kind (d) with 7 entries" % (case.name, case.reaches("c", 7), case.reaches("d", 7)))
    assert case.reaches("c", 7) >= 1 and case.reaches("d", 7) >= 1 and case.reaches("a") == 0, case.counts
    assert case.kept["len"].max() <= 8 and case.n_patterns <= 64
    check_host_helper(case)
    try:
        ctx.set_option("spmv_exact_public", 0)
        y, info = check_device_paths(ctx, case, 2, all_lds=True)
        assert info["rows_in_classes"] == case.n, info
    finally:
        restore(ctx)


def test_lattice_e_the_default_gates(fedd_lib, ctx):
    """the cube of 66 cells per side, Dirichlet on flag 2 only, spmv_pattern at its default: the classes are built because the
    system has 65 536 rows or more; lines of 65 non-Dirichlet rows give full 7-entry waves on one pattern (a), a Neumann face
    full 6-entry waves (e), and rows of 1, 4, 5, 6 and 7 entries exist"""
    case = Case(fedd_lib, ctx, "E", fedd_lib.structured_mesh(3, 1, 66), (2,), 4105)
    assert case.n == 300763 and case.reaches("a", 7) >= 1 and case.reaches("e", 6) >= 1, case.counts
    assert set(case.kept["len"].tolist()) >= {1, 4, 5, 6, 7} and case.kept["len"].max() <= 8 and case.n_patterns <= 64
    check_host_helper(case)
    need = classes_per_block(case.kept, case.n)
    blocks_a = sorted({w[1] // BLOCK_ROWS for w in of_kind(case.waves, "a", 7)})
    assert any(need[b] <= LDS_CAP_8 for b in blocks_a), need[blocks_a]      # a kind-(a) wave in a block with a list
    try:
        ctx.set_option("spmv_exact_public", 0)
        y, info = check_device_paths(ctx, case, 1)
        assert info["row_classes"] >= 1 and info["rows_in_classes"] == case.n, info
        assert info["class_blocks_fallback"] == np.count_nonzero(need > LDS_CAP_8), (info, np.sort(need)[-4:])
        check_planted_edge_lanes(case, y, "a", 7)
    finally:
        restore(ctx)


def test_a_solve_on_lattice_a_is_the_same_solve_on_the_three_paths(fedd_lib, ctx):
    """s-step GMRES (s = 16) with the one-level Schwarz preconditioner: solution, iteration count and gmres_info() bit for bit
    the same on the per-entry kernel, the class kernel and the class kernel with LDS lists; more than 16 iterations, so the
    shifted epilogue of the Newton basis (SpmvEpi) runs through the exchange branch.  Lattice A with Dirichlet values on every
    side converges in 14 iterations (a host restatement of the same preconditioned solve), so this is A's Neumann variant
    with one Dirichlet face (flag 2, x = 0): about a hundred."""
    case = Case(fedd_lib, ctx, "A one Dirichlet face", lattice(fedd_lib, "A"), (2,), 4106)
    assert case.reaches("a", 7) >= 1 and case.n_patterns <= 64, case.counts
    ctx.schwarz_set_target(27, 1.0)
    ctx.schwarz_setup(1, fedd_lib.COMBINE_RESTRICTED)
    try:
        ctx.set_option("gmres_s", 16)
        sol = {}
        for name, pattern, lds in (("per entry", 0, 1), ("classes", 2, 0), ("classes, LDS", 2, 1)):
            ctx.set_option("spmv_pattern", pattern)
            ctx.set_option("spmv_cls_lds", lds)
            xs, its, rel = ctx.gmres(None, rtol=1e-10, max_it=400, restart=100, use_prec=True)
            sol[name] = (xs, its, rel, ctx.gmres_info(), ctx.spmv_info())
            print("%s: %d iterations, relres %.3e, %s" % (name, its, rel, sol[name][3]))
        ref = sol["per entry"]
        assert ref[4]["row_classes"] == 0 and ref[1] > 16 and ref[3]["blocks"] >= 2 and ref[0].shape == (case.n,)
        assert sol["classes"][4]["row_classes"] >= 1 and sol["classes"][4]["class_blocks_lds"] == 0
        assert sol["classes, LDS"][4]["class_blocks_lds"] == case.nblk and sol["classes, LDS"][4]["class_blocks_fallback"] == 0
        for name in ("classes", "classes, LDS"):
            assert sol[name][1] == ref[1] and sol[name][2] == ref[2] and sol[name][3] == ref[3], name
            assert np.array_equal(sol[name][0], ref[0]), name
    finally:
        restore(ctx)
